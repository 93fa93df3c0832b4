"""`carpedeam contig_breaks` and `carpedeam ancient_assemble_fused --break-report` without a device: what the flag checks refuse before
a device is opened and before anything is written."""
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
    (tmp_path / "a.fq").write_text("@r\n" + "ACGT" * 10 + "\n+\n" + "I" * 40 + "\n")
    return tmp_path


def run(args, exe=EXE, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    # (no device is needed for any of these; where a machine has some, they are hidden, so that a check that came too late would show)
    e.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([exe] + args, capture_output=True, text=True, env=e, timeout=120)


OUT_OF_RANGE = [("--break-anchor", "0"), ("--break-anchor", "1025"), ("--break-edge", "0"), ("--break-edge", "1048577"), ("--min-span", "0"), ("--min-span", "1000001"),
                ("--min-span-percent", "-1"), ("--min-span-percent", "101"), ("--min-piece", "0"), ("--min-piece", "1048577")]


def outputs(inputs):
    return [str(inputs / n) for n in ("out.tsv", "split.fa", "span.bedgraph")]


@pytest.mark.parametrize("flag,value", OUT_OF_RANGE, ids=["%s=%s" % fv for fv in OUT_OF_RANGE])
def test_threshold_out_of_range(inputs, flag, value):
    out, split, bed = outputs(inputs)
    r = run(["contig_breaks", str(inputs / "contigs.fa"), str(inputs / "a.fq"), out, "--split", split, "--span-track", bed, flag, value])
    assert r.returncode == 77 and "contig_breaks: %s %s" % (flag, value) in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(split) and not os.path.exists(bed)


@pytest.mark.parametrize("flags,edge", [(["--break-anchor", "20", "--break-edge", "19"], "19"), (["--break-anchor", "51"], "50"), (["--break-edge", "15"], "15")],
                         ids=["both", "anchor_above_the_default_edge", "edge_below_the_default_anchor"])
def test_an_edge_below_the_anchor(inputs, flags, edge):
    out, split, bed = outputs(inputs)
    r = run(["contig_breaks", str(inputs / "contigs.fa"), str(inputs / "a.fq"), out, "--split", split, "--span-track", bed] + flags)
    assert r.returncode == 77 and "contig_breaks: --break-edge %s" % edge in r.stderr and "--break-anchor" in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(split) and not os.path.exists(bed)


def test_the_front_end_owns_the_command(inputs):
    log = str(inputs / "dispatch.log")
    r = run(["contig_breaks", str(inputs / "contigs.fa"), str(inputs / "a.fq"), str(inputs / "out.tsv"), "--break-anchor", "1025"], exe=FRONT, CARPEDEAM_DISPATCH_LOG=log)
    assert r.returncode == 1 and "not handed to the reference binary" in r.stderr
    assert open(log).read().split() == ["refused", "contig_breaks"]
    r = run([], exe=FRONT)
    assert "contig_breaks" in r.stderr


def test_unknown_flag(inputs):
    r = run(["contig_breaks", str(inputs / "contigs.fa"), str(inputs / "a.fq"), str(inputs / "out.tsv"), "--depth-edge", "0"])
    assert r.returncode == 1 and 'Unrecognized parameter "--depth-edge"' in r.stderr
    assert not os.path.exists(inputs / "out.tsv")


def test_too_few_arguments():
    r = run(["contig_breaks", "contigs.fa", "out.tsv"])
    assert r.returncode == 1 and "Usage: carpedeam contig_breaks" in r.stderr


@pytest.mark.parametrize("flags,message", [(["--break-anchor", "1025"], "--break-anchor 1025"), (["--min-span-percent", "101"], "--min-span-percent 101"),
                                           (["--break-anchor", "30", "--break-edge", "29"], "--break-edge 29")], ids=["anchor", "percent", "edge_below_anchor"])
def test_fused_threshold_out_of_range(inputs, flags, message):
    tmp = str(inputs / "tmp")
    r = run(["ancient_assemble_fused", str(inputs / "a.fq"), str(inputs / "out.fa"), tmp, "--break-report", str(inputs / "b.tsv")] + flags)
    assert r.returncode == 77 and "ancient_assemble_fused: " + message in r.stderr, r.stderr
    assert not os.path.exists(tmp) and not os.path.exists(inputs / "b.tsv") and not os.path.exists(inputs / "out.fa")


def test_fused_takes_the_flags_and_no_split(inputs):
    flags = ["--break-report", str(inputs / "b.tsv"), "--break-anchor", "8", "--break-edge", "20", "--min-span", "2", "--min-span-percent", "10"]
    r = run(["ancient_assemble_fused", str(inputs / "a.fq"), str(inputs / "out.fa"), str(inputs / "tmp")] + flags, CDM_FUSED_DRY_RUN="1")
    assert r.returncode == 0, r.stderr
    plain = run(["ancient_assemble_fused", str(inputs / "a.fq"), str(inputs / "out.fa"), str(inputs / "tmp")], CDM_FUSED_DRY_RUN="1")
    assert plain.returncode == 0 and r.stdout == plain.stdout          # (the flags change nothing of the assembly's steps)
    r = run(["ancient_assemble_fused", str(inputs / "a.fq"), str(inputs / "out.fa"), str(inputs / "tmp"), "--split", str(inputs / "s.fa")] + flags, CDM_FUSED_DRY_RUN="1")
    assert r.returncode == 1 and 'Unrecognized parameter "--split"' in r.stderr          # (a split FASTA would be a second assembly output)
