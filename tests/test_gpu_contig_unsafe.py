"""ancient_contig_merge --unsafe 1 on the device (csrc/contigunsafe.hip): the counts against the majority-vote consensus of the extending
candidates (nuclassembleUtil.cpp:535-790, host/contigmerge.cpp unsafeConsensus / unsafeColumns), then the device queue.  Against the
oracle on the same DB files, against the host queue over a synthetic loop, with queries handed back, over several ranks, and on inputs
built here to force the kernel's paths.  The CPU test pins those built inputs to the reference's object code where it is built."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

from carpedeam_amd import capi, mmdb
from gpuutil import diff_keys, gold, run_oracle, seqdb_to_keyed
from stageflags import A_FLAGS, KC_FLAGS, R_FLAGS
from test_contig_phase import REF, ROOT, UNSAFE_CASES, cgold, unsafe_flags

EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam")
DEVICE_LAP = "queues + extension (device)"
UNSAFE_LAP = re.compile(r"unsafe consensus columns \(device\) [0-9.]+ s: (\d+) queries, (\d+) column records, (\d+) tiles, (\d+) queries handed back")


def ctx_with_damage(dhigh_prefix):
    ctx = capi.Ctx(0)
    ctx.damage_load(dhigh_prefix)
    return ctx


def unsafe_par(min_cov=5):
    par = capi.AncientParams.default()
    par.unsafe, par.min_cov_safe = 1, min_cov
    return par


def unsafe_laps(err):
    """the unsafe pass's laps in CDM_TIMING's output -> [(queries, column records, tiles, handed back)]"""
    return [tuple(int(x) for x in m.groups()) for m in UNSAFE_LAP.finditer(err)]


def module_merge(tmp_path, corr, aln, out, min_cov, dhigh_prefix, env=None):
    """the module binary on DB files, queue pinned to the device, CDM_TIMING on -> its stderr"""
    e = dict(os.environ, CDM_CONTIG_QUEUE="device", CDM_TIMING="1", **(env or {}))
    r = subprocess.run([EXE, "ancient_contig_merge", corr, aln, out, *unsafe_flags(min_cov), "--ancient-damage", dhigh_prefix, "--threads", "4"],
                       capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    assert DEVICE_LAP in r.stderr and unsafe_laps(r.stderr), r.stderr[-2000:]
    return r.stderr


# ------------------------------------------------------------------------------------------------ 1. the reference's inputs, through the C ABI
@pytest.mark.gpu
@pytest.mark.parametrize("name,step,min_cov", UNSAFE_CASES)
def test_unsafe_merge_on_the_device_equals_the_oracle(oracle_bin, dhigh_prefix, tmp_path, monkeypatch, capfd, name, step, min_cov):
    """Ctx.contig_merge with unsafe = 1 and the queue on the device: the unsafe pass runs, and the merged DB (wasExtended included) is
    the oracle's `ancient_contig_merge --unsafe 1` on the same DB files - and not the safe mode's"""
    t = lambda s: str(tmp_path / s)
    mmdb.write_from_keyed(t("corr"), cgold(name, "ccorr", step), mmdb.DBTYPE_NUCLEOTIDES)
    mmdb.write_from_keyed(t("aln"), cgold(name, "caln", step), mmdb.DBTYPE_ALIGNMENT_RES)
    run_oracle(oracle_bin, "ancient_contig_merge", t("corr"), t("aln"), t("o"), *unsafe_flags(min_cov), "--ancient-damage", dhigh_prefix, "--threads", "2")
    monkeypatch.setenv("CDM_CONTIG_QUEUE", "device")
    monkeypatch.setenv("CDM_TIMING", "1")
    ctx = ctx_with_damage(dhigh_prefix)
    corr = ctx.upload_keyed_seqdb(cgold(name, "ccorr", step))
    aoff, arec = capi.parse_aln_db(cgold(name, "caln", step), corr.meta()[1])
    capfd.readouterr()
    merged = ctx.contig_merge(corr, ctx.upload_alns(corr, aoff, arec), unsafe_par(min_cov))
    err = capfd.readouterr().err
    assert DEVICE_LAP in err
    laps = unsafe_laps(err)
    assert len(laps) == 1 and laps[0][1] > 0, err
    if name != "letters":       # (with letters beyond ACGTN, the queries that hold them take the host code)
        assert laps[0][3] == 0 and "queues + extension (host)" not in err, err
    got = seqdb_to_keyed(*merged.download())
    assert not diff_keys(got, mmdb.read_db(t("o")))
    assert diff_keys(got, cgold(name, "cmerge", step))


# ------------------------------------------------------------------------------------------------ 2. device queue = host queue over a loop
def unsafe_loop(ctx, n, seed, iters_reads, iters_contigs, monkeypatch, where):
    """the workflow loop through the C ABI, the contig merges in unsafe mode -> the DB after every contig iteration"""
    monkeypatch.setenv("CDM_CONTIG_QUEUE", where)
    db = ctx.synth(n, 60, 150, seed)
    kp = capi.KmerParams.reads_default()
    kc = capi.KmerParams.reads_default()
    kc.kmer_size, kc.include_only_extendable = 22, 1
    par = capi.AncientParams.default()
    par.max_seq_len = 200000
    upar = unsafe_par()
    upar.max_seq_len = 200000
    out = []
    for it in range(iters_reads + iters_contigs):
        alns = ctx.rescore(db, ctx.kmermatch(db, kp if it < iters_reads else kc))
        corr = ctx.correct(db, alns, par)
        if it < iters_reads:
            db = ctx.extend(corr, alns, par)
        else:
            db = ctx.contig_merge(corr, alns, upar)
            lens, _, ext = db.meta()
            out.append((db.download()[0], lens.copy(), ext.copy()))
    return out


@pytest.mark.gpu
def test_seven_unsafe_contig_iterations_device_against_host(dhigh_prefix, monkeypatch):
    """200 000 mixed-length reads, 5 read + 7 contig iterations in unsafe mode: letters, lengths and flags after every contig
    iteration, device queue against host queue; contigs beyond 1 000 letters take several tiles of the consensus"""
    ctx = ctx_with_damage(dhigh_prefix)
    dev = unsafe_loop(ctx, 200_000, 2, 5, 7, monkeypatch, "device")
    host = unsafe_loop(ctx, 200_000, 2, 5, 7, monkeypatch, "host")
    grew = 0
    for it, ((d, dl, de), (h, hl, he)) in enumerate(zip(dev, host)):
        assert np.array_equal(dl, hl), it
        assert np.array_equal(de, he), it
        assert d == h, it
        grew += int(de.sum())
    assert grew > 10_000 and int(dev[-1][1].max()) > 1000


# ------------------------------------------------------------------------------------------------ 3. queries handed back
@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 3])
def test_unsafe_queries_handed_back_equal_the_oracle(oracle_bin, dhigh_prefix, tmp_path, every):
    """CDM_CONTIG_HAND_BACK_EVERY=k in unsafe mode: the host code takes every k-th query, the device the rest - same DB as the oracle"""
    t = lambda s: str(tmp_path / s)
    name, step, min_cov = "mixed3k", 1, 5
    mmdb.write_from_keyed(t("corr"), cgold(name, "ccorr", step), mmdb.DBTYPE_NUCLEOTIDES)
    mmdb.write_from_keyed(t("aln"), cgold(name, "caln", step), mmdb.DBTYPE_ALIGNMENT_RES)
    run_oracle(oracle_bin, "ancient_contig_merge", t("corr"), t("aln"), t("o"), *unsafe_flags(min_cov), "--ancient-damage", dhigh_prefix, "--threads", "2")
    err = module_merge(tmp_path, t("corr"), t("aln"), t("g"), min_cov, dhigh_prefix, {"CDM_CONTIG_HAND_BACK_EVERY": str(every)})
    assert "queries handed back to the host" in err
    assert not diff_keys(mmdb.read_db(t("g")), mmdb.read_db(t("o")))


@pytest.mark.gpu
@pytest.mark.parametrize("min_cov", [1, 5])
def test_unsafe_letters_beyond_acgtn_are_handed_back(oracle_bin, dhigh_prefix, tmp_path, min_cov):
    """the fuzz case with lower-case / IUPAC contigs (tests/golden/fuzzcases) in unsafe mode: the queries whose columns hold such a
    letter go to the host code (the lap counts them), the result is the oracle's"""
    t = lambda s: str(tmp_path / s)
    mmdb.write_from_keyed(t("in"), mmdb.load_keyed(os.path.join(ROOT, "tests", "golden", "fuzzcases", "contig_ga_letters.keyed.gz")), mmdb.DBTYPE_NUCLEOTIDES)
    dmg = ["--ancient-damage", dhigh_prefix, "--threads", "2"]
    run_oracle(oracle_bin, "kmermatcher", t("in"), t("pref"), *KC_FLAGS, "--threads", "1")
    run_oracle(oracle_bin, "rescorediagonal", t("in"), t("in"), t("pref"), t("aln"), *R_FLAGS, "--threads", "2")
    run_oracle(oracle_bin, "ancient_correction", t("in"), t("aln"), t("corr"), *unsafe_flags(min_cov), *dmg)
    run_oracle(oracle_bin, "ancient_contig_merge", t("corr"), t("aln"), t("o"), *unsafe_flags(min_cov), *dmg)
    err = module_merge(tmp_path, t("corr"), t("aln"), t("g"), min_cov, dhigh_prefix)
    (laps,) = unsafe_laps(err)
    assert laps[3] > 0, err
    assert not diff_keys(mmdb.read_db(t("g")), mmdb.read_db(t("o")))
    assert diff_keys(mmdb.read_db(t("g")), mmdb.read_db(t("corr")))


# ------------------------------------------------------------------------------------------------ 4. inputs built to force the kernel's paths
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(s):
    return s.translate(COMP)[::-1]


def built_case(kind, seed=7):
    """A query contig Q (key 0) cut from a random genome, and targets cut around its ends - their overlap with Q letter-exact, their
    extension mutated - with Q's alignment records written out directly (the other sequences have none).  -> (sequences, alignments,
    --min-cov-safe).  kind:
      deep      330 right and 40 left extenders: a pile-up deeper than the kernel's LDS list of contributors (256 per batch)
      mincov0/1 --min-cov-safe 0 / 1: every covered position votes; 0 also lets an uncovered one through to the tie rule
      mincovbig --min-cov-safe above the coverage: the flanks are all N, the columns come from the middle third alone
      ties      pairs of extenders that disagree letter for letter: tied columns (N)
      revn      reverse-oriented extenders (records with qStart > qEnd) carrying N letters in their extensions
    No target reaches beyond the consensus' 3 qLen letters: the reference writes behind its coverage vector there and dies of it (as
    the oracle does), so there is no result to match."""
    rng = random.Random(seed)
    genome = bytes(rng.choice(b"ACGT") for _ in range(6000))
    q0, qlen = 2000, 600
    query = genome[q0:q0 + qlen]
    mutated = lambda s, rate, n_rate=0.0: bytes((ord("N") if rng.random() < n_rate else rng.choice(b"ACGT")) if rng.random() < rate + n_rate else c for c in s)
    seqs, recs = {0: query}, []
    min_cov = {"mincov0": 0, "mincov1": 1, "mincovbig": 1000}.get(kind, 2)

    def add(left, qs_or_qe, length, rev=False, rate=0.1, n_rate=0.0, ext=None):
        key = len(seqs)
        if left:            # the target ends inside Q: qs = 0, de = tLen - 1
            e = q0 + qs_or_qe + 1
            s = e - length
            ext_part = ext if ext is not None else mutated(genome[s:q0], rate, n_rate)
            t = ext_part + genome[q0:e]
            qs, qe, ds, de = 0, qs_or_qe, len(ext_part), len(t) - 1
        else:               # the target starts inside Q: ds = 0, qe = qLen - 1
            length = min(length, qlen - qs_or_qe + qlen)          # (its letters end by 3 qLen)
            s = q0 + qs_or_qe
            ext_part = ext if ext is not None else mutated(genome[q0 + qlen:s + length], rate, n_rate)
            t = genome[s:q0 + qlen] + ext_part
            qs, qe, ds, de = qs_or_qe, qlen - 1, 0, qlen - 1 - qs_or_qe
        tlen = len(t)
        if rev:             # stored reverse-complemented: the record's query coordinates swap, its target's are the stored sequence's
            t = revcomp(t)
            qs, qe, ds, de = qe, qs, tlen - 1 - de, tlen - 1 - ds
        seqs[key] = t
        recs.append("%d\t%d\t1.000\t1.000E-100\t%d\t%d\t%d\t%d\t%d\t%d" % (key, 300, qs, qe, qlen, ds, de, tlen))

    if kind == "deep":
        for i in range(330):
            add(False, 100 + (i * 7) % 380, 500 + (i * 13) % 300, rev=(i % 5 == 0))
        for i in range(40):
            add(True, 250 + (i * 11) % 300, 400 + (i * 17) % 300)
    elif kind == "ties":
        for i in range(6):
            ext = bytes(rng.choice(b"ACGT") for _ in range(200))
            other = bytes(rng.choice([c for c in b"ACGT" if c != b]) for b in ext)
            add(False, 150 + 40 * i, 450 - 40 * i + 200, ext=ext)
            add(False, 150 + 40 * i, 450 - 40 * i + 200, ext=other)
            add(True, 300 + 20 * i, 300 + 20 * i + 200, ext=ext)
            add(True, 300 + 20 * i, 300 + 20 * i + 200, ext=other)
    elif kind == "revn":
        for i in range(12):
            add(False, 120 + 30 * i, 400 + 25 * i, rev=True, rate=0.05, n_rate=0.08)
            add(True, 250 + 25 * i, 380 + 20 * i, rev=True, rate=0.05, n_rate=0.08)
            add(False, 140 + 30 * i, 420 + 25 * i, rate=0.05)
    else:                   # mincov*: a moderate pile-up with uneven depth
        for i in range(24):
            add(False, 100 + 17 * i, 450 + 23 * i, rev=(i % 3 == 0))
            add(True, 200 + 15 * i, 350 + 19 * i, rev=(i % 4 == 1))
    alns = {k: (b"", 0) for k in seqs}
    alns[0] = (("\n".join(recs) + "\n").encode(), 0)
    return {k: (s + b"\n", 0) for k, s in seqs.items()}, alns, min_cov


BUILT = ["deep", "mincov0", "mincov1", "mincovbig", "ties", "revn"]


def write_built(tmp_path, kind):
    seqs, alns, min_cov = built_case(kind)
    t = lambda s: str(tmp_path / s)
    mmdb.write_from_keyed(t("corr"), seqs, mmdb.DBTYPE_NUCLEOTIDES)
    mmdb.write_from_keyed(t("aln"), alns, mmdb.DBTYPE_ALIGNMENT_RES)
    return t, min_cov


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref (the reference's object code) is not built here")
@pytest.mark.parametrize("kind", [k for k in BUILT if k != "mincov0"])          # (the reference refuses --min-cov-safe 0)
def test_oracle_on_built_unsafe_inputs_against_reference_binary(oracle_bin, dhigh_prefix, tmp_path, kind):
    """the inputs the device tests below force paths with: the oracle is the reference's object code on them, and Q grows (but where
    the extenders tie letter for letter)"""
    t, min_cov = write_built(tmp_path, kind)
    for exe, out in ((oracle_bin, "o"), (REF, "r")):
        run_oracle(exe, "ancient_contig_merge", t("corr"), t("aln"), t(out), *unsafe_flags(min_cov), "--ancient-damage", dhigh_prefix, "--threads", "2")
    o = mmdb.canon(mmdb.read_db(t("o")))
    assert o == mmdb.canon(mmdb.read_db(t("r")))
    assert kind == "ties" or len(o[0][0]) > 600


@pytest.mark.gpu
@pytest.mark.parametrize("kind", BUILT)
def test_unsafe_merge_on_built_inputs_equals_the_oracle(oracle_bin, dhigh_prefix, tmp_path, kind):
    """each built input (see built_case) through the module binary with the queue on the device, against the oracle"""
    t, min_cov = write_built(tmp_path, kind)
    run_oracle(oracle_bin, "ancient_contig_merge", t("corr"), t("aln"), t("o"), *unsafe_flags(min_cov), "--ancient-damage", dhigh_prefix, "--threads", "2")
    err = module_merge(tmp_path, t("corr"), t("aln"), t("g"), min_cov, dhigh_prefix)
    (laps,) = unsafe_laps(err)
    assert laps[0] == 1 and laps[3] == 0, err
    if kind == "deep":
        assert laps[2] > 1, err                     # the query's hull spans several tiles
    assert not diff_keys(mmdb.read_db(t("g")), mmdb.read_db(t("o")))


# ------------------------------------------------------------------------------------------------ 5./6. the module binary
@pytest.mark.gpu
@pytest.mark.parametrize("name,step,min_cov", [("synth2k", 0, 2), ("letters", 1, 2)])
def test_unsafe_module_on_db_files_equals_the_oracle(oracle_bin, dhigh_prefix, tmp_path, name, step, min_cov):
    """`carpedeam ancient_contig_merge --unsafe 1` with CDM_CONTIG_QUEUE=device on DB files"""
    t = lambda s: str(tmp_path / s)
    mmdb.write_from_keyed(t("corr"), cgold(name, "ccorr", step), mmdb.DBTYPE_NUCLEOTIDES)
    mmdb.write_from_keyed(t("aln"), cgold(name, "caln", step), mmdb.DBTYPE_ALIGNMENT_RES)
    run_oracle(oracle_bin, "ancient_contig_merge", t("corr"), t("aln"), t("o"), *unsafe_flags(min_cov), "--ancient-damage", dhigh_prefix, "--threads", "2")
    module_merge(tmp_path, t("corr"), t("aln"), t("g"), min_cov, dhigh_prefix)
    assert not diff_keys(mmdb.read_db(t("g")), mmdb.read_db(t("o")))


@pytest.mark.gpu
def test_unsafe_reads_loop_equals_the_oracle_chain(oracle_bin, dhigh_prefix, tmp_path):
    """`ancient_reads_loop --unsafe 1 --num-iter-reads-only 3 --num-iterations 5`, contig queue on the device, against the oracle's
    modules chained over the same five iterations in unsafe mode"""
    t = lambda s: str(tmp_path / s)
    mmdb.write_from_keyed(t("in"), gold("mixed3k", "reads"), mmdb.DBTYPE_NUCLEOTIDES)
    e = dict(os.environ, CDM_CONTIG_QUEUE="device", CDM_TIMING="1")
    r = subprocess.run([EXE, "ancient_reads_loop", t("in"), t("out"), "--ancient-damage", dhigh_prefix, "--num-iter-reads-only", "3", "--num-iterations", "5",
                        "--unsafe", "1", "--min-cov-safe", "2"], capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(unsafe_laps(r.stderr)) == 2, r.stderr[-2000:]
    au = " ".join(A_FLAGS).replace("--unsafe 0", "--unsafe 1").replace("--min-cov-safe 5", "--min-cov-safe 2").split()
    from stageflags import K_FLAGS
    cur = t("in")
    for it in range(5):
        kf, af = (K_FLAGS, au) if it < 3 else (KC_FLAGS, unsafe_flags(2))
        run_oracle(oracle_bin, "kmermatcher", cur, t("p"), *kf, "--threads", "4")
        run_oracle(oracle_bin, "rescorediagonal", cur, cur, t("p"), t("a"), *R_FLAGS, "--threads", "4")
        run_oracle(oracle_bin, "ancient_correction", cur, t("a"), t("c"), *af, "--ancient-damage", dhigh_prefix, "--threads", "4")
        run_oracle(oracle_bin, "ancient_read_assemble" if it < 3 else "ancient_contig_merge", t("c"), t("a"), t("n%d" % it), *af, "--ancient-damage", dhigh_prefix, "--threads", "4")
        cur = t("n%d" % it)
    assert not diff_keys(mmdb.read_db(t("out")), mmdb.read_db(cur))


# ------------------------------------------------------------------------------------------------ 7. over ranks
@pytest.mark.gpu
@pytest.mark.parametrize("world,transport", [(2, "threads"), (3, "standin")])
def test_unsafe_contig_iteration_over_ranks_equals_single_device(dhigh_prefix, world, transport, monkeypatch):
    """cdm_contig_iteration_dist with unsafe = 1 on `world` ranks sharing the device: corrected DB, merged DB and wasExtended flags of
    two contig iterations equal the single-device calls'"""
    from test_gpu_shards import run_native_ranks, run_standin_ranks
    monkeypatch.setenv("CDM_CONTIG_QUEUE", "device")
    capi.lib().cdm_env_refresh()
    n = 60_000
    kc = capi.KmerParams.reads_default()
    kc.kmer_size, kc.include_only_extendable = 22, 1
    par = unsafe_par()

    def start(c):
        db = c.synth(n, 60, 150, 3)
        for _ in range(3):
            alns = c.rescore(db, c.kmermatch(db))
            db = c.extend(c.correct(db, alns), alns)
        return db

    ref = ctx_with_damage(dhigh_prefix)
    db = start(ref)
    want = []
    for _ in range(2):
        alns = ref.rescore(db, ref.kmermatch(db, kc))
        corr = ref.correct(db, alns, par)
        db = ref.contig_merge(corr, alns, par)
        want.append((corr.download(), db.download()))
    assert int(want[1][1][2].sum()) > 1000
    del db, corr, alns

    def rank_fn(rank, comm, c):
        c.damage_load(dhigh_prefix)
        d = start(c)
        got = []
        for _ in range(2):
            _, corr, d = comm.contig_iteration(d, kc, apar=par)
            got.append((corr.download(), d.download()))
        return got

    res = (run_native_ranks if transport == "threads" else run_standin_ranks)(world, rank_fn)
    for r in res:
        for it in range(2):
            for got, exp in zip(r[it], want[it]):
                assert [bytes(x) for x in got[0]] == [bytes(x) for x in exp[0]]
                assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
