"""`carpedeam contig_depth` and `carpedeam ancient_assemble_fused --depth-report` without a device: what the flag checks refuse before a
device is opened and before anything is written."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


@pytest.fixture()
def inputs(tmp_path):
    (tmp_path / "contigs.fa").write_text(">c1\n" + "ACGT" * 20 + "\n")
    for name in ("a.fq", "b.fq"):
        (tmp_path / name).write_text("@r\n" + "ACGT" * 10 + "\n+\n" + "I" * 40 + "\n")
    return tmp_path


def run(args, exe=EXE, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    # (no device is needed for any of these; where a machine has some, they are hidden, so that a check that came too late would show)
    e.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([exe] + args, capture_output=True, text=True, env=e, timeout=120)


@pytest.mark.parametrize("edge", ["-1", "1048577"])
def test_depth_edge_out_of_range(inputs, edge):
    out = str(inputs / "out.tsv")
    r = run(["contig_depth", str(inputs / "contigs.fa"), str(inputs / "a.fq"), out, "--depth-edge", edge])
    assert r.returncode == 77 and "--depth-edge " + edge in r.stderr, r.stderr
    assert not os.path.exists(out)


def test_the_front_end_owns_the_command(inputs):
    log = str(inputs / "dispatch.log")
    r = run(["contig_depth", str(inputs / "contigs.fa"), str(inputs / "a.fq"), str(inputs / "out.tsv"), "--depth-edge", "-1"], exe=FRONT, CARPEDEAM_DISPATCH_LOG=log)
    assert r.returncode == 1 and "not handed to the reference binary" in r.stderr
    assert open(log).read().split() == ["refused", "contig_depth"]


def test_unknown_flag(inputs):
    r = run(["contig_depth", str(inputs / "contigs.fa"), str(inputs / "a.fq"), str(inputs / "out.tsv"), "--shuffle", "0"])
    assert r.returncode == 1 and 'Unrecognized parameter "--shuffle"' in r.stderr
    assert not os.path.exists(inputs / "out.tsv")


def test_the_track_takes_one_read_set(inputs):
    out, track = str(inputs / "out.tsv"), str(inputs / "out.bedgraph")
    r = run(["contig_depth", str(inputs / "contigs.fa"), str(inputs / "a.fq"), str(inputs / "b.fq"), out, "--depth-track", track])
    assert r.returncode == 77 and "--depth-track" in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(track)


def test_too_few_arguments():
    r = run(["contig_depth", "contigs.fa", "out.tsv"])
    assert r.returncode == 1 and "Usage: carpedeam contig_depth" in r.stderr


def test_fused_depth_edge_out_of_range(inputs):
    tmp = str(inputs / "tmp")
    r = run(["ancient_assemble_fused", str(inputs / "a.fq"), str(inputs / "out.fa"), tmp, "--depth-report", str(inputs / "d.tsv"), "--depth-edge", "-1"])
    assert r.returncode == 77 and "ancient_assemble_fused: --depth-edge -1" in r.stderr, r.stderr
    assert not os.path.exists(tmp) and not os.path.exists(inputs / "d.tsv")


def test_fused_takes_both_flags(inputs):
    r = run(["ancient_assemble_fused", str(inputs / "a.fq"), str(inputs / "out.fa"), str(inputs / "tmp"), "--depth-report", str(inputs / "d.tsv"), "--depth-edge", "7"], CDM_FUSED_DRY_RUN="1")
    assert r.returncode == 0, r.stderr
