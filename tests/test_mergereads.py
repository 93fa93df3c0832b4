"""mergereads (paired-end input, csrc/pairmerge.hip + host/main.cpp) without a device: the CPU restatement against the reference's
outputs, the front end's routing, the errors the module gives before any device is opened, and ancient_reads_loop's paired input."""
import gzip
import json
import os
import subprocess

import pytest

import pairmerge_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
MODULES = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
GOLD = os.path.join(ROOT, "tests", "golden", "mergereads")
CASES = {"adna100": ["R1", "R2"], "adna150": ["R1", "R2"], "letters": ["R1", "R2"], "long": ["R1", "R2"], "example": ["R1", "R2"],
         "two": ["A_R1", "A_R2", "B_R1", "B_R2"]}


def case_files(name):
    return [os.path.join(GOLD, "%s.%s.fq.gz" % (name, f)) for f in CASES[name]]


def built():
    from carpedeam_amd import build
    build.build()


def run(args, **kw):
    env = dict(os.environ, CDM_NO_FORK="1")
    env.pop("CARPEDEAM_REF_BIN", None)
    env.update(kw.pop("env", {}))
    return subprocess.run(args, capture_output=True, text=True, env=env, **kw)


def write_fq(path, recs):
    open(path, "w").write("".join("@%s\n%s\n+\n%s\n" % r for r in recs))


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_the_reference_outputs(name):
    files = case_files(name)
    entries = model.mergereads(list(zip(files[0::2], files[1::2])))
    assert model.digests(model.db_files(entries)) == json.load(open(os.path.join(GOLD, "digests.json")))[name]


def test_model_keyed_dump_agrees():
    # (the dumps are for diagnosis; one cross-check keeps them honest)
    entries = model.mergereads([tuple(case_files("letters"))])
    dump = gzip.open(os.path.join(GOLD, "letters.keyed.gz"), "rb").read().decode("latin-1").splitlines()
    assert [l.split("\t") for l in dump] == [[str(k), n.decode("latin-1"), s.decode("latin-1")] for k, (n, s) in enumerate(entries)]


def test_front_end_routes_mergereads_to_the_device_binary(tmp_path):
    built()
    stand_in = tmp_path / "modules.sh"
    stand_in.write_text('#!/bin/sh\necho "device $*"\n')
    stand_in.chmod(0o755)
    log = str(tmp_path / "dispatch.log")
    r = run([FRONT, "mergereads", "a.fq", "b.fq", "out"], env={"CARPEDEAM_GPU_BIN": str(stand_in), "CARPEDEAM_REF_BIN": "/bin/echo", "CARPEDEAM_DISPATCH_LOG": log})
    assert r.returncode == 0 and r.stdout == "device mergereads a.fq b.fq out\n"
    assert open(log).read().split() == ["gpu", "mergereads"]
    r = run([FRONT])
    assert " mergereads" in r.stderr.splitlines()[1]


def test_mergereads_errors_before_any_device(tmp_path):
    built()
    a, b, fa = str(tmp_path / "a.fq"), str(tmp_path / "b.fq"), str(tmp_path / "c.fa")
    write_fq(a, [("r1", "ACGTACGTACGTACGTACGTAAAA", "I" * 24)])
    write_fq(b, [("r1", "TTTTACGTACGTACGTACGTACGT", "I" * 24)])
    open(fa, "w").write(">x\nACGT\n")
    out = str(tmp_path / "out")
    # the reference's flag table (onlythreads): anything else is unrecognized, --compressed included
    r = run([MODULES, "mergereads", a, b, out, "--compressed", "1"])
    assert r.returncode == 1 and 'Unrecognized parameter "--compressed"' in r.stderr
    # a FASTA record has no quality
    r = run([MODULES, "mergereads", a, fa, out])
    assert r.returncode == 1 and "Invalid quality record found" in r.stderr
    # an empty sequence
    write_fq(str(tmp_path / "e.fq"), [("r1", "", "")])
    r = run([MODULES, "mergereads", str(tmp_path / "e.fq"), b, out])
    assert r.returncode == 1 and "Invalid sequence record found" in r.stderr
    # an odd number of inputs: the reference pairs the last one with its output DB, which is not there
    r = run([MODULES, "mergereads", a, b, a, out])
    assert r.returncode == 1 and out + ": No such file or directory" in r.stderr
    assert not any(os.path.exists(out + s) for s in ("", ".index", "_h", "_h.index"))
    # ... and when it is there, the reference would read it as the last R2 while writing it: refused (77), the file left alone
    open(out, "w").write("old")
    r = run([MODULES, "mergereads", a, b, a, out])
    assert r.returncode == 77 and "odd number of input files" in r.stderr and open(out).read() == "old"
    os.remove(out)
    # --threads / -v are accepted (then, without a device, the module stops at the device)
    r = run([MODULES, "mergereads", a, b, out, "--threads", "2", "-v", "3"])
    assert "Unrecognized" not in r.stderr and "Invalid" not in r.stderr


def test_reads_loop_takes_pairs_and_leaves_r2_alone(tmp_path, dhigh_prefix):
    built()
    a, b, fa = str(tmp_path / "a.fq"), str(tmp_path / "b.fq"), str(tmp_path / "c.fa")
    write_fq(a, [("r1", "ACGTACGTACGTACGTACGTAAAA", "I" * 24)])
    open(fa, "w").write(">x\nACGT\n")
    before = open(fa, "rb").read()
    out = str(tmp_path / "out")
    # R1 R2 OUT: the pairs are read (R2 here is FASTA: mergereads' error), R2 is an input and stays as it is
    r = run([MODULES, "ancient_reads_loop", a, fa, out, "--ancient-damage", dhigh_prefix])
    assert r.returncode == 1 and "Invalid quality record found" in r.stderr
    assert open(fa, "rb").read() == before and not os.path.exists(out)
    # an odd number of read files
    write_fq(b, [("r1", "TTTTACGTACGTACGTACGTACGT", "I" * 24)])
    r = run([MODULES, "ancient_reads_loop", a, b, a, out, "--ancient-damage", dhigh_prefix])
    assert r.returncode == 1 and "3 read files given" in r.stderr
    # --gpus > 1 with paired input: refused (77) before anything is read
    r = run([MODULES, "ancient_reads_loop", a, b, out, "--ancient-damage", dhigh_prefix, "--gpus", "2"])
    assert r.returncode == 77 and "--gpus > 1 with paired-end input" in r.stderr
