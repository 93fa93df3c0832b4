"""`carpedeam contig_depth`, `contig_variants` and `contig_breaks` with --gapped, without a device: what the flag checks refuse before a
device is opened and before anything is written, the usage lines, and what the binding declares.  The rules are contig_map's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
COMMANDS = ["contig_depth", "contig_variants", "contig_breaks"]
# the files a command can write beside its table
EXTRA = {"contig_depth": [("--depth-track", "out.bg")], "contig_variants": [("--sites", "out.sites"), ("--consensus", "out.fa")],
         "contig_breaks": [("--split", "out.fa"), ("--span-track", "out.bg")]}


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


def command(module, inputs, *flags):
    extra = [x for flag, name in EXTRA[module] for x in (flag, str(inputs / name))]
    return [module, str(inputs / "contigs.fa"), str(inputs / "a.fq"), str(inputs / "out.tsv")] + extra + list(flags)


def nothing_written(inputs):
    return sorted(os.listdir(inputs)) == ["a.fq", "contigs.fa"]


@pytest.mark.parametrize("module", COMMANDS)
def test_the_usage_line_names_the_flags(module):
    r = run([module, "contigs.fa", "out.tsv"])
    assert r.returncode == 1 and "Usage: carpedeam " + module in r.stderr
    for flag in ("--gapped 0", "--gap-band 8", "--gap-min-columns 32"):
        assert flag in r.stderr


@pytest.mark.parametrize("module", COMMANDS)
@pytest.mark.parametrize("flags", [("--gapped", "2"), ("--gapped", "-1"), ("--gapped", "1", "--gap-band", "0"), ("--gapped", "1", "--gap-band", "32"),
                                   ("--gapped", "1", "--gap-min-columns", "0"), ("--gapped", "1", "--gap-min-columns", "4097")], ids=lambda f: " ".join(f))
def test_values_out_of_range(inputs, module, flags):
    r = run(command(module, inputs, *flags))
    assert r.returncode == 77 and "%s: %s %s" % ((module,) + flags[-2:]) in r.stderr, r.stderr
    assert nothing_written(inputs)


@pytest.mark.parametrize("module", COMMANDS)
@pytest.mark.parametrize("flags", [("--gap-band", "8"), ("--gap-min-columns", "32"), ("--gapped", "0", "--gap-band", "4"), ("--gapped", "0", "--gap-min-columns", "40")], ids=lambda f: " ".join(f))
def test_a_gap_flag_without_gapped(inputs, module, flags):
    r = run(command(module, inputs, *flags))
    assert r.returncode == 77 and module + ": " in r.stderr and "without --gapped 1" in r.stderr, r.stderr
    assert nothing_written(inputs)


@pytest.mark.parametrize("module", COMMANDS)
@pytest.mark.parametrize("flags", [("--gapped", "0"), ("--gapped", "1"), ("--gapped", "1", "--gap-band", "31", "--gap-min-columns", "4096"), ("--gapped", "1", "--gap-band", "1", "--gap-min-columns", "1")],
                         ids=lambda f: " ".join(f))
def test_values_in_range_get_as_far_as_the_device(inputs, module, flags):
    """in range, the flags pass the checks and the command goes on to open the device, which these tests hide"""
    r = run(command(module, inputs, *flags))
    assert r.returncode not in (0, 77) and "Unrecognized" not in r.stderr and "not supported" not in r.stderr, r.stderr


def test_contig_damage_does_not_take_the_flag(inputs):
    r = run(["contig_damage", str(inputs / "contigs.fa"), str(inputs / "a.fq"), str(inputs / "out.tsv"), "--gapped", "1"])
    assert r.returncode == 1 and 'Unrecognized parameter "--gapped"' in r.stderr and nothing_written(inputs)


def test_the_binding_declares_the_calls():
    import inspect

    from carpedeam_amd import capi
    for name in ("cdm_pileup_depth_gapped", "cdm_pileup_bases_gapped", "cdm_pileup_breaks_gapped"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    for call in (capi.Ctx.pileup_depth, capi.Ctx.pileup_bases, capi.Ctx.pileup_breaks):
        assert inspect.signature(call).parameters["gapped"].default is None
