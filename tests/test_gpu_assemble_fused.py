"""`carpedeam ancient_assemble_fused` on the device, through the front end and with no reference binary anywhere: reads in, contig
FASTA out, against the FASTA files the reference's whole program wrote for the same reads and flags (tests/golden/example,
tests/golden/mergereads, tests/golden/fused - the last made by tests/golden/make_fused_golden.py, which keeps an input only when two
runs of the reference agree byte for byte).  No difference is tolerated."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLD, "fused", "cases.json")))


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


def fasta_records(data):
    recs = []
    for line in data.decode().split("\n"):
        if line.startswith(">"):
            recs.append([line, ""])
        elif recs:
            recs[-1][1] += line
    return recs


def assemble(tmp_path, dhigh_prefix, case, extra=(), env=None):
    c = CASES[case]
    log, out, tmp = str(tmp_path / "dispatch.log"), str(tmp_path / "out.fasta"), str(tmp_path / "tmp")
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(CARPEDEAM_DISPATCH_LOG=log, **(env or {}))
    r = subprocess.run([FRONT, "ancient_assemble_fused"] + [os.path.join(GOLD, p) for p in c["inputs"]] + [out, tmp, "--ancient-damage", dhigh_prefix, "--threads", "8"] + c["flags"] + list(extra),
                       capture_output=True, text=True, env=e, timeout=300)
    assert r.returncode == c["exit_status"], (r.stdout[-1500:], r.stderr[-1500:])
    assert open(log).read() == "gpu ancient_assemble_fused\n"          # one call, on the device: nothing else was started through the front end
    got, want = open(out, "rb").read(), open(os.path.join(GOLD, c["fasta"]), "rb").read()
    assert len(want) == c["fasta_bytes"]
    return got, want, r, tmp


def test_example_reads(tmp_path, dhigh_prefix):
    got, want, r, _ = assemble(tmp_path, dhigh_prefix, "example")
    assert fasta_records(got) == fasta_records(want)          # records, order, headers
    assert got == want
    assert "STEP: 9" in r.stderr and "STEP: 10" not in r.stderr          # the workflow's defaults: 5 read + 5 contig iterations


def test_example_pairs_with_min_contig_len_30(tmp_path, dhigh_prefix):
    got, want, _, _ = assemble(tmp_path, dhigh_prefix, "example_pairs_min30")
    assert got == want and got.count(b">") == 1148


def test_example_pairs_with_the_default_min_contig_len_keep_nothing(tmp_path, dhigh_prefix):
    """the hole of the drop-in workflow (linclust's kmermatcher on an empty DB): the reference's whole program ends with status 0 and an
    empty FASTA, and so does this command - linclust is not run on nothing"""
    got, want, r, _ = assemble(tmp_path, dhigh_prefix, "example_pairs_default")
    assert got == want == b"" and "0 assembled contigs" in r.stderr


def test_two_file_pairs(tmp_path, dhigh_prefix):
    got, want, _, _ = assemble(tmp_path, dhigh_prefix, "two")
    assert got == want and got.count(b">") == 5


def test_circular_contigs_reach_the_headers(tmp_path, dhigh_prefix):
    got, want, r, _ = assemble(tmp_path, dhigh_prefix, "circ")
    assert got == want
    assert b"cycle:1" in got and b"cycle:0" in got and "circular contigs set aside" in r.stderr


def test_non_default_flags_and_removed_tmp_files(tmp_path, dhigh_prefix):
    got, want, _, tmp = assemble(tmp_path, dhigh_prefix, "example_flags", extra=["--remove-tmp-files", "1"])
    assert got == want and got.count(b">") == 196
    assert os.listdir(tmp) == []                              # the command's own directory under <tmpDir> is gone


def test_flags_that_do_and_do_not_reach_linclust(tmp_path, dhigh_prefix):
    """-e, --hash-shift and -v change the loop and stop in front of linclust; --zdrop, --clust-min-cov and --max-seq-len go into it"""
    got, want, _, _ = assemble(tmp_path, dhigh_prefix, "example_tail")
    assert got == want and got.count(b">") == 96


def test_two_ranks_give_the_same_fasta(tmp_path, dhigh_prefix):
    """--gpus 2 (the library's RCCL transport over its in-process stand-in, one device): the loop over two ranks, rank 0 keeps the source
    index and the circular contigs, the tail runs on rank 0"""
    got, want, r, _ = assemble(tmp_path, dhigh_prefix, "circ", extra=["--gpus", "2"], env={"CDM_LOOP_TRANSPORT": "standin"})
    assert "on 2 ranks" in r.stderr and "circular contigs set aside" in r.stderr
    assert got == want and b"cycle:1" in got
