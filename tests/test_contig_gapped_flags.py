"""`carpedeam contig_map --gapped` without a device: what the flag checks refuse before a device is opened and before anything is
written, and what the binding declares."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def run(args, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    # (no device is needed for any of these; where a machine has some, they are hidden, so that a check that came too late would show)
    e.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=e, timeout=120)


def command(inputs, *flags):
    return ["contig_map", str(inputs / "contigs.fa"), str(inputs / "a.fq"), str(inputs / "out.sam")] + list(flags)


def test_the_usage_line_names_the_flags():
    r = run(["contig_map", "contigs.fa", "out.sam"])
    assert r.returncode == 1 and "Usage: carpedeam contig_map" in r.stderr
    for flag in ("--read-group", "--primary-only", "--gapped 0", "--gap-band 8", "--gap-min-columns 32"):
        assert flag in r.stderr


@pytest.mark.parametrize("flags", [("--gapped", "2"), ("--gapped", "-1"), ("--gapped", "1", "--gap-band", "0"), ("--gapped", "1", "--gap-band", "32"),
                                   ("--gapped", "1", "--gap-min-columns", "0"), ("--gapped", "1", "--gap-min-columns", "4097")], ids=lambda f: " ".join(f))
def test_values_out_of_range(inputs, flags):
    r = run(command(inputs, *flags))
    assert r.returncode == 77 and "contig_map: %s %s" % flags[-2:] in r.stderr, r.stderr
    assert not os.path.exists(inputs / "out.sam")


@pytest.mark.parametrize("flags", [("--gap-band", "8"), ("--gap-min-columns", "32"), ("--gapped", "0", "--gap-band", "4")], ids=lambda f: " ".join(f))
def test_a_gap_flag_without_gapped(inputs, flags):
    r = run(command(inputs, *flags))
    assert r.returncode == 77 and "without --gapped 1" in r.stderr, r.stderr
    assert not os.path.exists(inputs / "out.sam")


def test_the_binding_declares_the_calls():
    from carpedeam_amd import capi
    assert "cdm_pileup_gapped" in capi.EXPORTS and "cdm_gap_free" in capi.EXPORTS
    assert capi.GAP_DTYPE.itemsize == 64 and capi.GAP_DTYPE.names[-3:] == ("score", "ops", "words")
    assert hasattr(capi.lib(), "cdm_pileup_gapped") and hasattr(capi.lib(), "cdm_gap_free")
    import ctypes
    assert ctypes.sizeof(capi.GapRec) == 64 and ctypes.sizeof(capi.GapParams) == 36
