"""`carpedeam contig_map` without a device: what the flag checks refuse before a device is opened and before anything is written."""
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
    return ["contig_map", str(inputs / "contigs.fa"), str(inputs / "a.fq"), str(inputs / "out.sam")] + list(flags)


def test_too_few_arguments():
    r = run(["contig_map", "contigs.fa", "out.sam"])
    assert r.returncode == 1 and "Usage: carpedeam contig_map" in r.stderr and "--read-group" in r.stderr and "--primary-only" in r.stderr


@pytest.mark.parametrize("value", ["2", "-1"])
def test_primary_only_out_of_range(inputs, value):
    r = run(command(inputs, "--primary-only", value))
    assert r.returncode == 77 and "contig_map: --primary-only %s" % value in r.stderr, r.stderr
    assert not os.path.exists(inputs / "out.sam")


@pytest.mark.parametrize("value", ["", "a\tb"], ids=["empty", "tab"])
def test_a_read_group_sam_cannot_hold(inputs, value):
    r = run(command(inputs, "--read-group", value))
    assert r.returncode == 77 and "contig_map: --read-group" in r.stderr, r.stderr
    assert not os.path.exists(inputs / "out.sam")


def test_unknown_flag(inputs):
    r = run(command(inputs, "--break-anchor", "16"))
    assert r.returncode == 1 and 'Unrecognized parameter "--break-anchor"' in r.stderr
    assert not os.path.exists(inputs / "out.sam")


def test_the_front_end_owns_the_command(inputs):
    log = str(inputs / "dispatch.log")
    r = run(command(inputs, "--primary-only", "2"), exe=FRONT, CARPEDEAM_DISPATCH_LOG=log)
    assert r.returncode == 1 and "not handed to the reference binary" in r.stderr
    assert open(log).read().split() == ["refused", "contig_map"]
    r = run([], exe=FRONT)
    assert "contig_map" in r.stderr


def test_the_binding_declares_the_call():
    from carpedeam_amd import capi
    assert "cdm_pileup_map" in capi.EXPORTS and "cdm_map_free" in capi.EXPORTS
    assert capi.MAP_DTYPE.itemsize == 40 and (capi.MAP_REVERSE, capi.MAP_SECONDARY) == (1, 2)
    assert hasattr(capi.lib(), "cdm_pileup_map")
