"""--dedup on the contig_* commands and the contig_dedup command without a device: the refusals come with status 77 before a device is
opened and before anything is written, the two commands that do not take the flag do not recognise it, and contig_dedup's usage line
names the five commands that do."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")

IO = ["contigs.fa", "reads.fq", "out"]
TAKE = ["contig_damage", "contig_depth", "contig_variants", "contig_breaks", "contig_map"]
GAPPED = ["contig_depth", "contig_variants", "contig_breaks", "contig_map"]
USAGE = ("Usage: carpedeam contig_dedup <i:contigs DB|fast(a|q)[.gz]> <i:reads DB|fast(a|q)[.gz]> <o:tsvFile> [--min-seq-id 0.9] [-k 20] [--threads N]. "
         "The duplicate reads it counts are the ones that --dedup 1 leaves out of contig_damage, contig_depth, contig_variants, contig_breaks and contig_map.\n")


def run(args, cwd, exe=EXE):
    e = {k: v for k, v in os.environ.items() if k not in ("CARPEDEAM_REF_BIN", "CDM_TIMING", "CDM_FUSED_DRY_RUN")}
    # (no device is needed for any of these; where a machine has some, they are hidden, so that a check that came too late would show)
    e.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=e, cwd=cwd, timeout=120)
    return r.returncode, "".join(l for l in r.stderr.splitlines(True) if not l.startswith("Time for processing")), r.stdout


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


@pytest.mark.parametrize("module", TAKE)
@pytest.mark.parametrize("value", ["-1", "2"])
def test_outside_0_and_1_is_refused(module, value, tmp_path):
    status, stderr, stdout = run([module] + IO + ["--dedup", value], str(tmp_path))
    assert (status, stderr, stdout) == (77, "%s: --dedup %s is not supported by the MI355X path (0 counts every record, 1 leaves the duplicate reads out)\n" % (module, value), "")
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("module", GAPPED)
@pytest.mark.parametrize("order", [0, 1])
def test_dedup_with_gapped_is_refused_and_says_why(module, order, tmp_path):
    flags = [["--dedup", "1"], ["--gapped", "1"]]
    status, stderr, stdout = run([module] + IO + flags[order] + flags[1 - order], str(tmp_path))
    assert (status, stdout) == (77, "")
    assert stderr == ("%s: --dedup 1 with --gapped 1 is not supported by the MI355X path (rescue candidates are the hits without a record, so a removed record would be rescued, "
                      "and rescued reads need a duplicate rule of their own)\n" % module)
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("module", TAKE)
@pytest.mark.parametrize("flags", [["--dedup", "0"], ["--dedup", "1"], ["--dedup", "0", "--gapped", "1"], ["--dedup", "1", "--gapped", "0"]])
def test_accepted_values_get_as_far_as_the_device(module, flags, tmp_path):
    """(no device here: the command ends when it opens one, and not over its flags)"""
    if "--gapped" in flags and module not in GAPPED:
        flags = flags[:2]
    status, stderr, _ = run([module] + IO + flags, str(tmp_path))
    assert status == 1 and "Unrecognized" not in stderr and "not supported" not in stderr and "Usage" not in stderr and "no CPU fallback" in stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("args", [["contig_indels"] + IO, ["ancient_assemble_fused", "reads.fq", "out.fa", "tmp"]], ids=["contig_indels", "ancient_assemble_fused"])
def test_the_other_two_commands_do_not_know_the_flag(args, tmp_path):
    status, stderr, stdout = run(args + ["--dedup", "1"], str(tmp_path))
    assert (status, stderr, stdout) == (1, 'Unrecognized parameter "--dedup"\n', "")
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("args", [[], IO[:1], IO[:2], IO + ["extra"]], ids=["none", "one", "two", "four"])
def test_the_usage_line_of_contig_dedup(args, tmp_path):
    status, stderr, stdout = run(["contig_dedup"] + args, str(tmp_path))
    assert (status, stderr, stdout) == (1, USAGE, "")
    for module in TAKE:
        assert module in USAGE.split("--dedup 1")[1]
    assert os.listdir(tmp_path) == []


def test_contig_dedup_flags(tmp_path):
    status, stderr, _ = run(["contig_dedup"] + IO + ["--dedup", "1"], str(tmp_path))
    assert (status, stderr) == (1, 'Unrecognized parameter "--dedup"\n')
    status, stderr, _ = run(["contig_dedup"] + IO + ["--gapped", "1"], str(tmp_path))
    assert (status, stderr) == (1, 'Unrecognized parameter "--gapped"\n')
    status, stderr, _ = run(["contig_dedup"] + IO + ["--min-seq-id", "0.95", "-k", "18", "--threads", "2"], str(tmp_path))
    assert status == 1 and "Unrecognized" not in stderr and "Usage" not in stderr and "no CPU fallback" in stderr
    assert os.listdir(tmp_path) == []


def test_the_commands_are_listed(tmp_path):
    status, stderr, _ = run([], str(tmp_path))
    assert status == 1 and "|contig_indels|contig_dedup|" in stderr
    # the front end hands the command to the device binary, not to a reference binary
    log = tmp_path / "dispatch.log"
    e = dict(os.environ, CARPEDEAM_DISPATCH_LOG=str(log), HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    e.pop("CARPEDEAM_REF_BIN", None)
    r = subprocess.run([FRONT, "contig_dedup"], capture_output=True, text=True, env=e, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 1 and r.stderr.startswith("Usage: carpedeam contig_dedup")
    assert "contig_dedup" in log.read_text()
