"""The contig_join command without a device: its usage line, its refusals (status 77 before a device is opened and before anything is
written), the flags it does not know, the front end's dispatch, and the binding of cdm_pileup_junctions."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")

IO = ["contigs.fa", "reads.fq", "joins.tsv"]
USAGE = ("Usage: carpedeam contig_join <i:contigs DB|fast(a|q)[.gz]> <i:reads DB|fast(a|q)[.gz]> <o:tsvFile> [--joined <fastaFile>] [--paths <tsvFile>] [--join-overlap-percent 90] "
         "[--link-anchor 16] [--link-overhang 1] [--link-max-ends 16] [--min-link-reads 2] [--dedup 0] [--min-seq-id 0.9] [-k 20] [--threads N]\n")
REFUSED = [("--join-overlap-percent", ["-1", "101"], "a percentage of the overlap's columns is 0 to 100"),
           ("--link-anchor", ["0", "1025", "-3"], "an end record has 1 to 1024 columns on its contig"),
           ("--link-overhang", ["0", "1025"], "an end record's read has 1 to 1024 letters beyond the contig's end"),
           ("--link-max-ends", ["1", "65", "0"], "a read that makes links has 2 to 64 end records at the most"),
           ("--min-link-reads", ["0", "1000001"], "a link that is written has 1 to 1000000 reads at the least"),
           ("--dedup", ["-1", "2"], "0 counts every record, 1 leaves the duplicate reads out")]


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


@pytest.mark.parametrize("args", [[], IO[:1], IO[:2], IO + ["extra"]], ids=["none", "one", "two", "four"])
def test_the_usage_line(args, tmp_path):
    status, stderr, stdout = run(["contig_join"] + args, str(tmp_path))
    assert (status, stderr, stdout) == (1, USAGE, "")
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("flag,values,why", REFUSED, ids=[r[0] for r in REFUSED])
def test_values_out_of_range_are_refused(flag, values, why, tmp_path):
    for value in values:
        status, stderr, stdout = run(["contig_join"] + IO + ["--joined", "joined.fa", "--paths", "paths.tsv", flag, value], str(tmp_path))
        assert (status, stderr, stdout) == (77, "contig_join: %s %s is not supported by the MI355X path (%s)\n" % (flag, value, why), "")
        assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("flag", ["--gapped", "--gfa", "--ends", "--no-such-flag", "--gap-band"])
def test_flags_it_does_not_know(flag, tmp_path):
    """--gapped among them: the rescued reads are not covered; --gfa and --ends are contig_links' own"""
    status, stderr, stdout = run(["contig_join"] + IO + [flag, "1"], str(tmp_path))
    assert (status, stderr, stdout) == (1, 'Unrecognized parameter "%s"\n' % flag, "")
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("flags", [[], ["--join-overlap-percent", "0", "--link-anchor", "1", "--link-overhang", "1024", "--link-max-ends", "2", "--min-link-reads", "1000000"],
                                   ["--join-overlap-percent", "100", "--link-anchor", "1024", "--link-overhang", "1", "--link-max-ends", "64", "--min-link-reads", "1", "--dedup", "1"],
                                   ["--joined", "joined.fa", "--paths", "paths.tsv", "--dedup", "0", "--min-seq-id", "0.95", "-k", "18", "--threads", "2"]], ids=["none", "low", "high", "files"])
def test_accepted_values_get_as_far_as_the_device(flags, tmp_path):
    """(no device here: the command ends when it opens one, and not over its flags)"""
    status, stderr, _ = run(["contig_join"] + IO + flags, str(tmp_path))
    assert status == 1 and "Unrecognized" not in stderr and "not supported" not in stderr and "Usage" not in stderr and "no CPU fallback" in stderr
    assert os.listdir(tmp_path) == []


def test_the_command_is_listed_and_the_front_end_owns_it(tmp_path):
    status, stderr, _ = run([], str(tmp_path))
    assert status == 1 and "|contig_links|contig_join|" in stderr
    # the front end hands the command to the device binary, not to a reference binary
    log = tmp_path / "dispatch.log"
    e = dict(os.environ, CARPEDEAM_DISPATCH_LOG=str(log), HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    e.pop("CARPEDEAM_REF_BIN", None)
    r = subprocess.run([FRONT, "contig_join"], capture_output=True, text=True, env=e, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 1 and r.stderr == USAGE
    assert "contig_join" in log.read_text()


def test_the_binding_declares_the_call():
    import join_model
    from carpedeam_amd import capi
    assert capi.JUNCTION_DTYPE.itemsize == 16 and capi.JUNCTION_DTYPE == join_model.JUNCTION_DTYPE and capi.C.sizeof(capi.Junction) == 16
    assert capi.JUNCTION_RES_DTYPE.itemsize == 40 and capi.JUNCTION_RES_DTYPE == join_model.RES_DTYPE and capi.C.sizeof(capi.JunctionRes) == 40
    assert [f[0] for f in capi.JunctionRes._fields_] == list(capi.JUNCTION_RES_DTYPE.names) and capi.JUNCTION_RES_DTYPE.fields["fill_off"][1] == 16
    assert "cdm_pileup_junctions" in capi.EXPORTS and "cdm_junction_free" in capi.EXPORTS and capi.JUNCTION_CONTAINED == join_model.CONTAINED == 1
    lib = capi.lib()
    assert lib.cdm_pileup_junctions.argtypes is not None and len(lib.cdm_pileup_junctions.argtypes) == 12 and lib.cdm_junction_free.restype is None
