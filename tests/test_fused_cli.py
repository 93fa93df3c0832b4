"""`carpedeam ancient_assemble_fused` without a device: its arguments, its flag table, its refusals, and the parameter strings it derives
for the modules of its tail against those the reference's own drivers built (tests/golden/fused/calls_*.json, recorded from
oracle/_ref/carpedeam_full behind a logging front by tests/golden/make_fused_golden.py)."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
FUSED = os.path.join(ROOT, "tests", "golden", "fused")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example", "test_data.fq.gz")
CMD = "ancient_assemble_fused"


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


def run(args, exe=EXE, **env):
    e = {k: v for k, v in os.environ.items() if k != "CARPEDEAM_REF_BIN"}
    e.update(env)
    return subprocess.run([exe, CMD] + args, capture_output=True, text=True, env=e, timeout=120)


def test_usage_and_argument_counts(tmp_path):
    r = run([])
    assert r.returncode == 1 and "Usage: carpedeam ancient_assemble_fused" in r.stderr
    for args in (["reads.fq"], ["reads.fq", "out.fa"]):
        r = run(args)
        assert r.returncode == 1 and "Too few input files provided." in r.stderr
    # an odd number of read files other than one (GuidedNuclassembler.cpp:89-97)
    r = run(["a_1.fq", "a_2.fq", "b_1.fq", "out.fa", str(tmp_path / "tmp")])
    assert r.returncode == 1 and "Too many input files provided." in r.stderr
    assert not os.path.exists(str(tmp_path / "tmp"))          # nothing was touched


def test_unknown_flag():
    r = run(["reads.fq", "out.fa", "tmp", "--no-such-flag", "1"])
    assert r.returncode == 1 and 'Unrecognized parameter "--no-such-flag"' in r.stderr


@pytest.mark.parametrize("flag,value", [("--cluster-mode", "0"), ("--gap-open", "11"), ("--cov-mode", "0"), ("--gap-extend", "1"), ("-a", "1"), ("--compressed", "1")])
def test_values_this_path_does_not_compute_are_refused(tmp_path, flag, value):
    args = ["reads.fq", "out.fa", str(tmp_path / "tmp"), flag, value]
    r = run(args)
    assert r.returncode == 77 and ("ancient_assemble_fused: %s %s is not supported by the MI355X path" % (flag, value)) in r.stderr
    log = str(tmp_path / "dispatch.log")
    r = run(args, exe=FRONT, CARPEDEAM_DISPATCH_LOG=log)
    assert r.returncode == 1 and "not handed to the reference binary" in r.stderr
    assert open(log).read().split() == ["refused", CMD]
    assert not os.path.exists(str(tmp_path / "tmp"))


@pytest.mark.parametrize("flag,value", [("--cluster-mode", "2"), ("--cov-mode", "1"), ("--gap-open", "5"), ("--gap-extend", "2"), ("-a", "0"), ("--compressed", "0")])
def test_the_one_value_is_accepted(flag, value):
    r = run(["reads.fq", "out.fa", "tmp", flag, value], CDM_FUSED_DRY_RUN="1")
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("flag", ["-k", "--kmer-per-seq", "--sub-mat", "--mask", "--db-mode", "-c", "--wrapped-scoring"])
def test_flags_of_the_reference_workflow_that_are_not_handled_are_refused(flag):
    r = run(["reads.fq", "out.fa", "tmp", flag, "1"])
    assert r.returncode == 77 and flag + " is not supported by the MI355X path" in r.stderr


def test_existing_output_is_refused(tmp_path):
    out = tmp_path / "out.fa"
    out.write_text(">x\nACGT\n")
    r = run([EXAMPLE, str(out), str(tmp_path / "tmp")])
    assert r.returncode == 1 and "exists already!" in r.stderr
    assert out.read_text() == ">x\nACGT\n"


def test_without_a_device_the_library_says_so(tmp_path, dhigh_prefix):
    """(the devices of a machine that has some are hidden from the process: the reads are parsed, then the context fails)"""
    out = str(tmp_path / "out.fa")
    r = run([EXAMPLE, out, str(tmp_path / "tmp"), "--ancient-damage", dhigh_prefix], HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    assert r.returncode not in (0, 77), r.stderr[-800:]
    assert "Can not initialise the MI355X device" in r.stderr and "no CPU fallback" in r.stderr
    assert not os.path.exists(out)


def recorded_tail(case):
    """(the flags the reference was called with, its module calls from linclust on, the hashed directory under clu_tmp folded)"""
    calls = json.load(open(os.path.join(FUSED, "calls_%s.json" % case)))
    assert calls[0][:4] == ["ancient_assemble", "$IN0", "$OUT", "$TMPDIR"] and calls[1][0] == "linclust"
    tail = [[re.sub(r"^\$TMP/clu_tmp/\d+/", "$TMP/clu_tmp/", a) for a in c] for c in calls[1:]]
    return ["/somewhere/dhigh" if f == "$DAMAGE" else f for f in calls[0][4:]], tail


def dry_run(flags, cycle=False):
    r = run(["reads.fq", "out.fa", "tmp"] + flags, CDM_FUSED_DRY_RUN="cycle" if cycle else "1")
    assert r.returncode == 0, r.stderr
    assert not os.path.exists("tmp")
    return [l.split(" ") for l in r.stdout.split("\n") if l]


# example_tail: flags that reach linclust through CLUSTER_PAR (--zdrop, --clust-min-cov, --max-seq-len) and flags that do not (-e,
# --hash-shift, -v: linclust's modules run with its own defaults, the user's -v reaches the three modules behind it);
# circ: createhdb with the cycle DB
@pytest.mark.parametrize("case", ["example", "example_flags", "example_tail", "circ"])
def test_derived_parameter_strings_equal_the_reference_drivers(case):
    flags, want = recorded_tail(case)
    assert [c[0] for c in want] == ["linclust", "kmermatcher", "rescorediagonal", "clust", "createsubdb", "createsubdb", "filterdb", "align", "clust", "mergeclusters",
                                    "result2repseq", "createhdb", "convert2fasta"]
    got = dry_run(flags, cycle=case == "circ")
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (g[0], [x for x in zip(g, w) if x[0] != x[1]][:4])
    createhdb = [c for c in got if c[0] == "createhdb"][0]
    assert (createhdb[2] == "$TMP/nuclassembly_rep_cycle") == (case == "circ")


def test_threads_and_remove_tmp_files_travel_with_cluster_par():
    """--threads and --remove-tmp-files stand in CLUSTER_PAR (LocalParameters.h:208-209): the recorded strings with those two values changed"""
    flags, want = recorded_tail("example")
    flags = [{"8": "3"}.get(f, f) if flags[i - 1] == "--threads" else f for i, f in enumerate(flags)] + ["--remove-tmp-files", "1"]
    swap = lambda c: [("3" if c[i - 1] == "--threads" else "1" if c[i - 1] == "--remove-tmp-files" else a) if i else a for i, a in enumerate(c)]
    assert dry_run(flags) == [swap(c) for c in want]


def test_a_tmp_dir_with_white_space_is_refused(tmp_path):
    r = run(["reads.fq", "out.fa", str(tmp_path / "my tmp")])
    assert r.returncode == 1 and "white space" in r.stderr and not os.path.exists(str(tmp_path / "my tmp"))


def test_gpus_with_paired_end_input_is_refused_as_in_the_loop(tmp_path):
    args = ["a_1.fq", "a_2.fq", str(tmp_path / "out.fa"), str(tmp_path / "tmp"), "--gpus", "2"]
    r = run(args)
    assert r.returncode == 77 and "ancient_assemble_fused: --gpus > 1 with paired-end input is not supported by the MI355X path" in r.stderr
    assert not os.path.exists(str(tmp_path / "out.fa"))


def test_nothing_kept_fixture_says_what_the_reference_does():
    """with nothing selected the reference's whole program ends well and leaves an empty FASTA"""
    cases = json.load(open(os.path.join(FUSED, "cases.json")))
    c = cases["example_pairs_default"]
    assert c["exit_status"] == 0 and c["fasta_bytes"] == 0 and c["flags"] == []
    assert os.path.getsize(os.path.join(FUSED, "example_pairs_default.fasta")) == 0
