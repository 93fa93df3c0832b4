"""mergereads on the MI355X (csrc/pairmerge.hip): the module's DB files byte for byte against the reference's (tests/golden/mergereads),
the kernel against the CPU restatement (tests/pairmerge_model.py) on seeded random pairs in batches of any size, the refusal of quality
bytes >= 0x80, ancient_reads_loop's paired input, and - where oracle/_ref is built - the live reference and the paired-end workflow."""
import collections
import gzip
import hashlib
import json
import os
import random
import subprocess

import pytest

import pairmerge_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
MODULES = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
REF_FULL = os.path.join(ROOT, "oracle", "_ref", "carpedeam_full")
GOLD = os.path.join(ROOT, "tests", "golden", "mergereads")
FILES = ["", ".index", ".dbtype", "_h", "_h.index", "_h.dbtype"]
CASES = {"adna100": ["R1", "R2"], "adna150": ["R1", "R2"], "letters": ["R1", "R2"], "long": ["R1", "R2"], "example": ["R1", "R2"],
         "two": ["A_R1", "A_R2", "B_R1", "B_R2"]}
# what is left on the reference binary: its three workflow drivers
ON_REFERENCE = {"ancient_assemble": 1, "nuclassemble": 1, "linclust": 1}

pytestmark = pytest.mark.gpu


def case_files(name):
    return [os.path.join(GOLD, "%s.%s.fq.gz" % (name, f)) for f in CASES[name]]


def digests(out):
    return {s: hashlib.sha256(open(out + s, "rb").read()).hexdigest() for s in FILES}


def run(args, env=None, timeout=600):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run(args, capture_output=True, text=True, env=e, timeout=timeout)
    return r


@pytest.fixture(scope="module")
def built():
    from carpedeam_amd import build
    build.build()


@pytest.mark.parametrize("name", sorted(CASES))
def test_module_matches_the_reference_files(built, tmp_path, name):
    out = str(tmp_path / "out")
    r = run([MODULES, "mergereads"] + case_files(name) + [out])
    assert r.returncode == 0, r.stderr[-2000:]
    assert digests(out) == json.load(open(os.path.join(GOLD, "digests.json")))[name]
    assert not os.path.exists(out + ".lookup") and not os.path.exists(out + ".source")


def test_module_plain_files_parallel_parse_and_small_batches(built, tmp_path):
    # plain (not gzip) inputs parsed by all threads, and device batches of 7 pairs: the same files
    files = []
    for p in case_files("adna100"):
        q = str(tmp_path / os.path.basename(p)[:-3])
        open(q, "wb").write(gzip.open(p).read())
        files.append(q)
    out = str(tmp_path / "out")
    r = run([MODULES, "mergereads"] + files + [out, "--threads", "4"], env={"CDM_INGEST_PAR_MIN": "1", "CDM_MERGE_BATCH": "7", "CDM_TIMING": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert digests(out) == json.load(open(os.path.join(GOLD, "digests.json")))["adna100"]


def random_pairs(rng, n):
    """Pairs of every letter class of the contract: real overlaps, N-rich, lower case, IUPAC, '.'-bytes, ties, long overlaps, short reads."""
    pairs = []
    for k in range(n):
        kind = k % 8
        L = rng.choice([rng.randint(1, 40), rng.randint(30, 250), rng.randint(100, 700)])
        frag = bytes(rng.choice(b"ACGT") for _ in range(L))
        l1, l2 = rng.randint(1, max(1, min(L, 300))), rng.randint(1, max(1, min(L, 300)))
        if kind == 7:
            l1 = l2 = min(L, rng.randint(60, 700))
        s1, s2 = bytearray(frag[:l1]), bytearray(model.revcomp(frag, frag)[0][:l2])
        for s in (s1, s2):
            for i in range(len(s)):
                u = rng.random()
                if u < 0.02:
                    s[i] = rng.choice(b"ACGT")
                elif kind == 1 and u < 0.2:
                    s[i] = ord("N")
                elif kind == 2 and u < 0.1:
                    s[i] = s[i] | 0x20
                elif kind == 3 and u < 0.08:
                    s[i] = rng.choice(b"RYKMSWBDHVUrykn.-*#xX")
        lo, hi = (40, 42) if kind in (4, 5) else (33, 74)
        q1 = bytes(rng.randint(lo, hi) for _ in s1)
        q2 = bytes(rng.randint(lo, hi) for _ in s2)
        if kind == 6:
            s2 = bytearray(rng.choice(b"ACGT") for _ in s2)
        pairs.append(((bytes(s1), q1), (bytes(s2), q2)))
    return pairs


def test_kernel_equals_the_restatement_in_any_batch(built):
    from carpedeam_amd import capi
    ctx = capi.Ctx(0)
    rng = random.Random(7)
    pairs = random_pairs(rng, 3000)
    expect = []
    for (s1, q1), (s2, q2) in pairs:
        expect.append([s for _, s in model.merge_pair((b"a", s1, q1), (b"b", s2, q2))])
    for batch, upto in ((4096, len(pairs)), (7, len(pairs)), (1, 300)):
        got = []
        for lo in range(0, upto, batch):
            status, entries = ctx.merge_pairs(pairs[lo:lo + batch])
            it = iter(entries)
            for st in status:
                got.append([next(it)] if st else [next(it), next(it)])
        assert got == expect[:upto], batch
    # the same entries as a resident DB: keys from first_key, wasExtended 1
    status, db = ctx.merge_pairs(pairs[:500], to_seqdb=True, first_key=10)
    seqs, keys, ext = db.download()
    flat = [s for e in expect[:500] for s in e]
    assert [bytes(s) for s in seqs] == flat and list(keys) == list(range(10, 10 + len(flat))) and set(ext) == {1}
    # a 5 000-bp pair (beyond the LDS stage)
    frag = bytes(rng.choice(b"ACGT") for _ in range(5600))
    big = [((frag[:5000], b"I" * 5000), (model.revcomp(frag[600:], frag[600:])[0], b"5" * 5000))]
    assert ctx.merge_pairs(big)[1] == [s for _, s in model.merge_pair((b"a",) + big[0][0], (b"b",) + big[0][1])]


def test_density_bound_parameters(built):
    # no density bound to speak of: every shift walks its whole overlap - the same answer as the restatement, and it ends
    from carpedeam_amd import capi
    ctx = capi.Ctx(0)
    pairs = random_pairs(random.Random(11), 400)
    status, entries = ctx.merge_pairs(pairs, par=capi.MergeParams(15, 65, 1000.0))
    expect = [s for (s1, q1), (s2, q2) in pairs for _, s in model.merge_pair((b"a", s1, q1), (b"b", s2, q2), max_dens=1000.0)]
    assert entries == expect
    # no number, or beyond any overlap: refused before anything runs
    for bad in (float("inf"), float("nan"), 1e7, -0.5):
        with pytest.raises(capi.CdmError):
            ctx.merge_pairs(pairs[:5], par=capi.MergeParams(15, 65, bad))


def test_high_quality_bytes_are_refused(built, tmp_path):
    a, b = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    open(a, "wb").write(b"@r1\nACGTACGTACGTACGTACGTAAAA\n+\n" + b"I" * 23 + b"\x90\n")
    open(b, "wb").write(b"@r1\nTTTTACGTACGTACGTACGTACGT\n+\n" + b"I" * 24 + b"\n")
    out = str(tmp_path / "out")
    r = run([MODULES, "mergereads", a, b, out])
    assert r.returncode == 77 and "0x80" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
    from carpedeam_amd import capi
    with pytest.raises(capi.CdmError):
        capi.Ctx(0).merge_pairs([((b"ACGT" * 6, b"I" * 23 + b"\x90"), (b"ACGT" * 6, b"I" * 24))])


def test_reads_loop_paired_equals_mergereads_then_loop(built, tmp_path, dhigh_prefix):
    files = case_files("example")
    loop = ["--ancient-damage", dhigh_prefix, "--num-iter-reads-only", "2", "--num-iterations", "3"]
    db, out1, out2 = str(tmp_path / "db"), str(tmp_path / "o1"), str(tmp_path / "o2")
    r = run([MODULES, "mergereads"] + files + [db])
    assert r.returncode == 0, r.stderr[-2000:]
    r = run([MODULES, "ancient_reads_loop", db, out1] + loop)
    assert r.returncode == 0, r.stderr[-2000:]
    before = [open(f, "rb").read() for f in files]
    r = run([MODULES, "ancient_reads_loop"] + files + [out2, "--shuffle", "1"] + loop)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [open(f, "rb").read() for f in files] == before
    for s in ("", ".index", ".dbtype"):
        assert open(out1 + s, "rb").read() == open(out2 + s, "rb").read(), s


@pytest.mark.skipif(not os.path.exists(REF_FULL), reason="oracle/_ref (the reference's object code) is not built here")
def test_live_reference_gives_the_same_files(built, tmp_path):
    for name in ("letters", "two"):
        a, b = str(tmp_path / (name + "_dev")), str(tmp_path / (name + "_ref"))
        assert run([MODULES, "mergereads"] + case_files(name) + [a]).returncode == 0
        assert run([REF_FULL, "mergereads"] + case_files(name) + [b, "--threads", "1"]).returncode == 0
        assert digests(a) == digests(b)


@pytest.mark.skipif(not os.path.exists(REF_FULL), reason="oracle/_ref (the reference's object code) is not built here")
def test_paired_end_workflow(built, tmp_path, dhigh_prefix):
    # `carpedeam ancient_assemble R1 R2 ...` through the front end: the reference's drivers and scripts, mergereads and every other module
    # on the device binary; the reference's FASTA (make_mergereads_golden.py workflow: --min-contig-len 30, see there)
    log = str(tmp_path / "dispatch.log")
    env = {"CARPEDEAM_GPU_BIN": MODULES, "CARPEDEAM_REF_BIN": REF_FULL, "CARPEDEAM_DISPATCH_LOG": log}
    out = str(tmp_path / "out.fasta")
    r = run([FRONT, "ancient_assemble"] + case_files("example") + [out, str(tmp_path / "tmp"), "--ancient-damage", dhigh_prefix, "--threads", "8",
                                                                  "--min-contig-len", "30"], env=env, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    calls = collections.Counter(tuple(l.split()) for l in open(log))
    assert {m: c for (where, m), c in calls.items() if where == "ref"} == ON_REFERENCE          # nothing else runs on the reference
    assert calls[("gpu", "mergereads")] == 1 and calls[("gpu", "createdb")] == 0
    assert calls[("gpu", "ancient_correction")] == 10 and calls[("gpu", "kmermatcher")] == 11 and calls[("gpu", "convert2fasta")] == 1
    assert not [k for k in calls if k[0] in ("refused", "fallback")]
    assert open(out).read() == open(os.path.join(GOLD, "example_ancient_assemble.fasta")).read()
