"""The contig_links command without a device: its usage line, its refusals (status 77 before a device is opened and before anything is
written), the flags it does not know, the front end's dispatch, and the binding of cdm_pileup_links."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")

IO = ["contigs.fa", "reads.fq", "links.tsv"]
USAGE = ("Usage: carpedeam contig_links <i:contigs DB|fast(a|q)[.gz]> <i:reads DB|fast(a|q)[.gz]> <o:tsvFile> [--link-anchor 16] [--link-overhang 1] [--link-max-ends 16] "
         "[--min-link-reads 2] [--ends <tsvFile>] [--gfa <gfaFile>] [--dedup 0] [--min-seq-id 0.9] [-k 20] [--threads N]\n")
REFUSED = [("--link-anchor", ["0", "1025", "-3"], "an end record has 1 to 1024 columns on its contig"),
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
    status, stderr, stdout = run(["contig_links"] + args, str(tmp_path))
    assert (status, stderr, stdout) == (1, USAGE, "")
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("flag,values,why", REFUSED, ids=[r[0] for r in REFUSED])
def test_values_out_of_range_are_refused(flag, values, why, tmp_path):
    for value in values:
        status, stderr, stdout = run(["contig_links"] + IO + ["--ends", "ends.tsv", "--gfa", "graph.gfa", flag, value], str(tmp_path))
        assert (status, stderr, stdout) == (77, "contig_links: %s %s is not supported by the MI355X path (%s)\n" % (flag, value, why), "")
        assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("flag", ["--gapped", "--no-such-flag", "--gap-band", "--break-anchor"])
def test_flags_it_does_not_know(flag, tmp_path):
    """--gapped among them: the rescued reads are not covered"""
    status, stderr, stdout = run(["contig_links"] + IO + [flag, "1"], str(tmp_path))
    assert (status, stderr, stdout) == (1, 'Unrecognized parameter "%s"\n' % flag, "")
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("flags", [[], ["--link-anchor", "1", "--link-overhang", "1024", "--link-max-ends", "2", "--min-link-reads", "1000000"],
                                   ["--link-anchor", "1024", "--link-overhang", "1", "--link-max-ends", "64", "--min-link-reads", "1", "--dedup", "1"],
                                   ["--ends", "ends.tsv", "--gfa", "graph.gfa", "--dedup", "0", "--min-seq-id", "0.95", "-k", "18", "--threads", "2"]], ids=["none", "low", "high", "files"])
def test_accepted_values_get_as_far_as_the_device(flags, tmp_path):
    """(no device here: the command ends when it opens one, and not over its flags)"""
    status, stderr, _ = run(["contig_links"] + IO + flags, str(tmp_path))
    assert status == 1 and "Unrecognized" not in stderr and "not supported" not in stderr and "Usage" not in stderr and "no CPU fallback" in stderr
    assert os.listdir(tmp_path) == []


def test_the_command_is_listed_and_the_front_end_owns_it(tmp_path):
    status, stderr, _ = run([], str(tmp_path))
    assert status == 1 and "|contig_indels|contig_dedup|contig_links|" in stderr
    # the front end hands the command to the device binary, not to a reference binary
    log = tmp_path / "dispatch.log"
    e = dict(os.environ, CARPEDEAM_DISPATCH_LOG=str(log), HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    e.pop("CARPEDEAM_REF_BIN", None)
    r = subprocess.run([FRONT, "contig_links"], capture_output=True, text=True, env=e, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 1 and r.stderr == USAGE
    assert "contig_links" in log.read_text()


def test_the_binding_declares_the_call():
    import links_model
    from carpedeam_amd import capi
    assert capi.LINK_DTYPE.itemsize == 48 and capi.LINK_DTYPE == links_model.LINK_DTYPE and capi.C.sizeof(capi.Link) == 48
    assert capi.C.sizeof(capi.LinksParams) == 24 and [f[0] for f in capi.LinksParams._fields_] == ["anchor", "overhang", "max_ends", "min_reads", "min_seq_id", "skip_extended_targets"]
    assert "cdm_pileup_links" in capi.EXPORTS and "cdm_link_free" in capi.EXPORTS
    par = capi.LinksParams.default()
    assert (par.anchor, par.overhang, par.max_ends, par.min_reads) == tuple(links_model.DEFAULTS[k] for k in ("anchor", "overhang", "max_ends", "min_reads"))
    lib = capi.lib()
    assert lib.cdm_pileup_links.argtypes is not None and len(lib.cdm_pileup_links.argtypes) == 11 and lib.cdm_link_free.restype is None
