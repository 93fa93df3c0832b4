"""`carpedeam contig_variants` and `carpedeam ancient_assemble_fused --variant-report` without a device: what the flag checks refuse
before a device is opened and before anything is written."""
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


OUT_OF_RANGE = [("--mask-ends", "-1"), ("--mask-ends", "65"), ("--min-depth", "0"), ("--min-depth", "1000001"), ("--min-alt-count", "0"), ("--min-alt-count", "1000001"),
                ("--min-alt-percent", "-1"), ("--min-alt-percent", "101")]


@pytest.mark.parametrize("flag,value", OUT_OF_RANGE, ids=["%s=%s" % fv for fv in OUT_OF_RANGE])
def test_threshold_out_of_range(inputs, flag, value):
    out, sites, cons = (str(inputs / n) for n in ("out.tsv", "sites.tsv", "cons.fa"))
    r = run(["contig_variants", str(inputs / "contigs.fa"), str(inputs / "a.fq"), out, "--sites", sites, "--consensus", cons, flag, value])
    assert r.returncode == 77 and "contig_variants: %s %s" % (flag, value) in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(sites) and not os.path.exists(cons)


def test_the_front_end_owns_the_command(inputs):
    log = str(inputs / "dispatch.log")
    r = run(["contig_variants", str(inputs / "contigs.fa"), str(inputs / "a.fq"), str(inputs / "out.tsv"), "--mask-ends", "65"], exe=FRONT, CARPEDEAM_DISPATCH_LOG=log)
    assert r.returncode == 1 and "not handed to the reference binary" in r.stderr
    assert open(log).read().split() == ["refused", "contig_variants"]


def test_unknown_flag(inputs):
    r = run(["contig_variants", str(inputs / "contigs.fa"), str(inputs / "a.fq"), str(inputs / "out.tsv"), "--depth-edge", "0"])
    assert r.returncode == 1 and 'Unrecognized parameter "--depth-edge"' in r.stderr
    assert not os.path.exists(inputs / "out.tsv")


def test_too_few_arguments():
    r = run(["contig_variants", "contigs.fa", "out.tsv"])
    assert r.returncode == 1 and "Usage: carpedeam contig_variants" in r.stderr


def test_fused_mask_ends_out_of_range(inputs):
    tmp = str(inputs / "tmp")
    r = run(["ancient_assemble_fused", str(inputs / "a.fq"), str(inputs / "out.fa"), tmp, "--variant-report", str(inputs / "v.tsv"), "--variant-sites", str(inputs / "s.tsv"), "--mask-ends", "65"])
    assert r.returncode == 77 and "ancient_assemble_fused: --mask-ends 65" in r.stderr, r.stderr
    assert not os.path.exists(tmp) and not os.path.exists(inputs / "v.tsv") and not os.path.exists(inputs / "s.tsv")


def test_fused_takes_the_flags(inputs):
    flags = ["--variant-report", str(inputs / "v.tsv"), "--variant-sites", str(inputs / "s.tsv"), "--min-depth", "2", "--min-alt-count", "1", "--min-alt-percent", "10", "--mask-ends", "2"]
    r = run(["ancient_assemble_fused", str(inputs / "a.fq"), str(inputs / "out.fa"), str(inputs / "tmp")] + flags, CDM_FUSED_DRY_RUN="1")
    assert r.returncode == 0, r.stderr
    plain = run(["ancient_assemble_fused", str(inputs / "a.fq"), str(inputs / "out.fa"), str(inputs / "tmp")], CDM_FUSED_DRY_RUN="1")
    assert plain.returncode == 0 and r.stdout == plain.stdout          # (the flags change nothing of the assembly's steps)
