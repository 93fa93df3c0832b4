"""`carpedeam contig_indels` without a device: the usage line, what the flag checks refuse before a device is opened and before anything
is written, the front end's dispatch, and what the binding declares."""
import ctypes
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


def command(inputs, *flags):
    return ["contig_indels", str(inputs / "contigs.fa"), str(inputs / "a.fq"), str(inputs / "out.tsv")] + list(flags)


def outputs(inputs):
    return [f for f in os.listdir(inputs) if f not in ("contigs.fa", "a.fq")]


def test_the_usage_line_names_the_flags():
    r = run(["contig_indels", "contigs.fa", "out.tsv"])
    assert r.returncode == 1 and "Usage: carpedeam contig_indels" in r.stderr
    for flag in ("--min-depth 3", "--min-indel-count 2", "--min-indel-percent 20", "--gap-band 8", "--gap-min-columns 32", "--sites", "--consensus", "--min-seq-id 0.9", "-k 20", "--threads"):
        assert flag in r.stderr
    r = run([])
    assert "contig_indels" in r.stderr


@pytest.mark.parametrize("flag,value", [("--min-depth", "0"), ("--min-depth", "1000001"), ("--min-indel-count", "0"), ("--min-indel-count", "1000001"), ("--min-indel-percent", "-1"),
                                        ("--min-indel-percent", "101"), ("--gap-band", "0"), ("--gap-band", "32"), ("--gap-min-columns", "0"), ("--gap-min-columns", "4097")],
                         ids=lambda v: v)
def test_values_out_of_range(inputs, flag, value):
    r = run(command(inputs, flag, value, "--sites", str(inputs / "sites.tsv"), "--consensus", str(inputs / "polished.fa")))
    assert r.returncode == 77 and "contig_indels: %s %s" % (flag, value) in r.stderr, r.stderr
    assert outputs(inputs) == []


def test_the_gap_flags_need_no_other_flag(inputs):
    """the gapped alignment is always on here: in range, the two flags get as far as the device, which these tests hide"""
    r = run(command(inputs, "--gap-band", "4", "--gap-min-columns", "40"))
    assert r.returncode not in (0, 77) and "Unrecognized" not in r.stderr and "not supported" not in r.stderr
    assert outputs(inputs) == []


@pytest.mark.parametrize("flag", ["--gapped", "--min-alt-count", "--break-anchor"])
def test_unknown_flag(inputs, flag):
    r = run(command(inputs, flag, "1"))
    assert r.returncode == 1 and 'Unrecognized parameter "%s"' % flag in r.stderr
    assert outputs(inputs) == []


def test_the_front_end_owns_the_command(inputs):
    log = str(inputs / "dispatch.log")
    r = run(command(inputs, "--min-depth", "0"), exe=FRONT, CARPEDEAM_DISPATCH_LOG=log)
    assert r.returncode == 1 and "not handed to the reference binary" in r.stderr
    assert open(log).read().split() == ["refused", "contig_indels"]
    r = run([], exe=FRONT)
    assert "contig_indels" in r.stderr


def test_the_binding_declares_the_calls():
    from carpedeam_amd import capi
    assert "cdm_pileup_indels" in capi.EXPORTS and "cdm_indel_free" in capi.EXPORTS
    assert capi.INDEL_DTYPE.itemsize == 40 and capi.INDEL_DTYPE.names == ("query", "pos", "info", "count", "cross", "others", "n_letters", "reserved", "letters")
    assert hasattr(capi.lib(), "cdm_pileup_indels") and hasattr(capi.lib(), "cdm_indel_free")
    assert ctypes.sizeof(capi.IndelSite) == 40 and ctypes.sizeof(capi.IndelParams) == 20
    assert ctypes.sizeof(capi.GapRec) == 64 and ctypes.sizeof(capi.GapParams) == 36 and ctypes.sizeof(capi.MapRec) == 40
    assert hasattr(capi.Ctx, "pileup_indels")
