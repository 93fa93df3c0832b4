"""GPU parity of the slot layout's split of sort 1 (round 9: 27 k-mer bits through the global passes; the grouping kernel's group capacity
and largest sorting network are compile-time parameters of its instances): the hit lists of the default, of the split of the rounds before (CDM_SLOT_LOWBITS), of the
12-byte layout and of the all-global sort are the same, on small inputs that reach every path the split and the geometry touch."""
import os

import numpy as np
import pytest

from carpedeam_amd import capi, mmdb
from gpuutil import diff_keys, run_oracle
from stageflags import K_FLAGS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


def reads(n, L, seed, genome_len, copies=(), dup=0.0, lowc=0):
    """n reads of L letters from a random genome of genome_len letters (both strands); for every c in `copies` one read from outside the
    genome c times over - each of its k-mers has exactly c tuples, which is a bucket of c (30 k distinct k-mers in 2^27 buckets: no
    other k-mer shares one); `dup` verbatim repeats and `lowc` tandem repeats as in test_gpu_slotlayout.py"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    genome = rng.integers(0, 4, genome_len + L)
    out = []
    for _ in range(n):
        st = int(rng.integers(0, genome_len))
        c = genome[st:st + L].copy()
        if rng.random() < 0.5:
            c = (3 - c)[::-1]
        out.append(letters[c].tobytes().decode())
    for _ in range(int(dup * n)):
        out.append(out[int(rng.integers(0, n))])
    for c in copies:
        out += [letters[rng.integers(0, 4, L)].tobytes().decode()] * c
    units = ["ACGTTGCA", "AC", "A", "ACGTACGTAC", "TTGCAACG", "ACGGT"]
    for i in range(lowc):
        u = units[i % len(units)]
        out.append((u * (L // len(u) + 1))[:L])
    return [out[i] for i in rng.permutation(len(out))]


def arrays(ctx, db, par=None):
    off, rec = ctx.kmermatch(db, par).download()
    return off, rec


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def parent_split(k):
    return str(2 * k + 1 - 27)


# (L, k, n, genome, extras): every head segment is a partial tile at these sizes
SHAPES = {
    "plain": (100, 20, 3000, 15000, {}),
    # buckets of exactly 128 and 129 (the largest a wave finishes and the smallest for the list at CDM_BUCKET_CAP=128), 256 and 257 (the
    # same at the instance's own capacity) and 600 (past the 512-slot window of a wave that owns its start: second batch, bisection for
    # its end)
    "heavy": (100, 20, 3000, 15000, dict(copies=(128, 129, 256, 257, 600), dup=0.05, lowc=12)),
    "k14": (40, 14, 3000, 6000, dict(copies=(128, 129, 200), dup=0.05, lowc=6)),       # 1 low bit
    "k17": (60, 17, 3000, 9000, dict(copies=(128, 129, 200), dup=0.05, lowc=6)),       # 7 low bits
}

def keyed_db(ctx, seqs, tmp_path):
    mmdb.write_seqdb(str(tmp_path / "in"), seqs)
    keyed = mmdb.read_db(str(tmp_path / "in"))
    return keyed, ctx.upload_keyed_seqdb(keyed)


@pytest.fixture(scope="module")
def dbs(ctx, tmp_path_factory):
    out = {}
    for name, (L, k, n, G, kw) in SHAPES.items():
        seqs = reads(n, L, seed=1000 + L + k, genome_len=G, **kw)
        d = tmp_path_factory.mktemp(name)
        keyed, db = keyed_db(ctx, seqs, d)
        par = capi.KmerParams(k, 200, 0.2, 67, 1, 0, 1, 0.0)
        old = os.environ.get("CDM_KMER_LAYOUT")
        os.environ["CDM_KMER_LAYOUT"] = "packed"
        try:
            ref = arrays(ctx, db, par)
        finally:
            if old is None:
                del os.environ["CDM_KMER_LAYOUT"]
            else:
                os.environ["CDM_KMER_LAYOUT"] = old
        assert len(ref[1]) > n      # (hits beyond the self hits)
        out[name] = dict(seqs=seqs, keyed=keyed, db=db, par=par, k=k, ref=ref, dir=d)
    return out


def run(ctx, monkeypatch, d, env):
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    try:
        return arrays(ctx, d["db"], d["par"])
    finally:
        for key in env:
            monkeypatch.delenv(key)


@pytest.mark.parametrize("name", list(SHAPES))
def test_default_parent_split_packed_and_lsd_agree(ctx, dbs, monkeypatch, name):
    d = dbs[name]
    assert capi.kmer_slot_split(d["k"]) == max(0, 2 * d["k"] - 27)
    for env in ({}, {"CDM_KMER_LAYOUT": "slot"}, {"CDM_SLOT_LOWBITS": parent_split(d["k"])}, {"CDM_KMER_SORT": "lsd"}, {"CDM_SLOT_HIST": "check"}):
        assert same(run(ctx, monkeypatch, d, env), d["ref"]), env


def test_heavy_shape_against_the_oracle(ctx, dbs, oracle_bin, monkeypatch):
    d = dbs["heavy"]
    t = lambda s: str(d["dir"] / s)
    run_oracle(oracle_bin, "kmermatcher", t("in"), t("pref"), *K_FLAGS, "--threads", "4")
    want = {key: (v[0], 0) for key, v in mmdb.read_db(t("pref")).items()}
    _, keys, _ = d["db"].meta()
    off, rec = run(ctx, monkeypatch, d, {})
    assert not diff_keys({key: (v, 0) for key, v in capi.hits_to_text(off, rec, keys).items()}, want)


@pytest.mark.parametrize("name", ["heavy", "k14", "k17"])
def test_bucket_capacities_around_128(ctx, dbs, monkeypatch, name):
    """the buckets of 128, 129 and more tuples against a capacity of 128, one below, one above, half, the instance's own 256 and one
    beyond it (clamped): below the group capacity of 256 a group of several buckets can hold one that is too long for the wave, which the
    walk has to find; the same with the split of the rounds before, where two k-mers can share a bucket"""
    d = dbs[name]
    for cap in ("128", "127", "129", "64", "256", "300", "1"):
        for split in (None, parent_split(d["k"])):
            env = {"CDM_BUCKET_CAP": cap}
            if split is not None:
                env["CDM_SLOT_LOWBITS"] = split
            assert same(run(ctx, monkeypatch, d, env), d["ref"]), env


@pytest.mark.parametrize("name", ["plain", "heavy"])
def test_small_owned_range_and_record_overflow(ctx, dbs, monkeypatch, name):
    """40 owned slots per wave and a stage of 2 run records: records cross rows of one group and overflow to the list"""
    d = dbs[name]
    for env in ({"CDM_BUCKET_CAP": "512,40", "CDM_REC_LIMIT": "2"}, {"CDM_BUCKET_CAP": "128,40", "CDM_REC_LIMIT": "2"}, {"CDM_BUCKET_CAP": "100,17", "CDM_REC_LIMIT": "0"},
                {"CDM_REC_LIMIT": "2"}, {"CDM_RUN_RECORDS": "kernel"}, {"CDM_BUCKET_CAP": "512,40", "CDM_REC_LIMIT": "2", "CDM_SLOT_LOWBITS": parent_split(d["k"])}):
        assert same(run(ctx, monkeypatch, d, env), d["ref"]), env


def test_wide_key_behind_the_new_split(ctx, dbs, monkeypatch):
    d = dbs["heavy"]
    wide = run(ctx, monkeypatch, d, {"CDM_FORCE_WIDE_KEY": "1"})
    assert same(wide, d["ref"])
    assert same(run(ctx, monkeypatch, d, {"CDM_FORCE_WIDE_KEY": "1", "CDM_BUCKET_CAP": "127,40"}), d["ref"])


def test_other_splits_the_passes_serve(ctx, dbs, monkeypatch):
    """every split with at most two passes behind the head digit gives the same hits (k = 17: 7 .. 25 low bits would do, the 64-bit sort word from 16 on)"""
    d = dbs["k17"]
    for n in (7, 9, 15, 16):
        assert same(run(ctx, monkeypatch, d, {"CDM_SLOT_LOWBITS": str(n)}), d["ref"]), n


def test_a_split_the_passes_do_not_serve_is_refused(ctx, dbs, monkeypatch):
    d = dbs["plain"]
    for n in ("12", "32", "-1", "x"):
        with pytest.raises(capi.CdmError) as e:
            run(ctx, monkeypatch, d, {"CDM_SLOT_LOWBITS": n})
        assert "CDM_SLOT_LOWBITS" in str(e.value)
    assert same(run(ctx, monkeypatch, d, {}), d["ref"])
