"""cdm_pileup_profile and cdm_seqdb_concat on the device against tests/pileup_model.py: alignment sets built by hand
(tests/pileupcases.py) and entered through cdm_alns_upload, random sets, the refusals, and the synth2k reads through cdm_kmermatch and
cdm_rescore.  Every comparison is between integers and exact."""
import numpy as np
import pytest

import pileup_model as pm
import pileupcases as pc
from carpedeam_amd import capi, mmdb
from gpuutil import gold

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


def device(ctx, c, queries=None):
    db = ctx.upload_seqs(c["seqs"], ext=c["ext"])
    alns = ctx.upload_alns(db, c["off"], c["rec"])
    return ctx.pileup_profile(db, alns, c["queries"] if queries is None else queries, c["ends"], c["min_seq_id"], c["skip"])


def model(c):
    return pm.profile(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"], c["ends"], c["min_seq_id"], c["skip"])


def assert_same(got, want, what=""):
    for g, w, name in zip(got, want, ("counts", "reads", "columns")):
        assert g.dtype == np.uint64 and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].tolist())


@pytest.mark.parametrize("name,make", pc.DIRECTED, ids=[n for n, _ in pc.DIRECTED])
def test_directed_cases(ctx, name, make):
    c = make()
    want = model(c)
    assert_same(device(ctx, c), want, name)
    if name == "query_lists":           # the query with only its identity record: all zeros
        k = c["queries"].index(7)
        assert want[0][k].sum() == 0 and want[1][k] == 0 and want[2][k] == 0


def test_one_record_more_than_a_chunk(ctx):
    """a pile-up of chunk + 1 records takes two work items whose tables meet in the query's row"""
    chunk = capi.pileup_chunk_records()
    assert 1 <= chunk <= 1 << 20
    c = pc.depth(chunk + 1)
    assert len(c["rec"]) == chunk + 2
    assert_same(device(ctx, c), model(c))


def test_small_chunks_and_launch_slices(ctx, monkeypatch):
    """the same tables when a query's records are cut into many items (3 records each) and the items into several launches"""
    c = pc.depth(129)
    want = model(c)
    before = capi.pileup_chunk_records()
    monkeypatch.setenv("CDM_PILEUP_CHUNK", "3")
    monkeypatch.setenv("CDM_LAUNCH_SLICE", "5")
    assert capi.pileup_chunk_records() == 3
    assert_same(device(ctx, c), want)
    q = pc.query_lists()
    assert_same(device(ctx, q), model(q))
    monkeypatch.delenv("CDM_PILEUP_CHUNK")
    monkeypatch.delenv("CDM_LAUNCH_SLICE")
    assert capi.pileup_chunk_records() == before


def test_the_empty_query_list(ctx):
    c = pc.query_lists()
    counts, reads, columns = device(ctx, c, queries=[])
    assert counts.shape == (0, 2, 16, 4, 4) and len(reads) == 0 and len(columns) == 0


def test_random_sets(ctx):
    """200 random sets; per set a random subset of up to 4 queries in random order is profiled (every record of the set is uploaded;
    the model's time goes with the records it walks, and the whole file is to take a few seconds)"""
    counted = 0
    for seed in range(200):
        c = pc.random_set(10_000 + seed, max_queries=4)
        want = model(c)
        assert_same(device(ctx, c), want, "seed %d" % seed)
        counted += int(want[1].sum())
    assert counted > 10_000


def test_refusals(ctx):
    c = pc.one_query_of_40()
    db = ctx.upload_seqs(c["seqs"])
    alns = ctx.upload_alns(db, c["off"], c["rec"])
    for ends in (0, 65, -1):
        with pytest.raises(capi.CdmError, match="cdm error -3.*ends"):
            ctx.pileup_profile(db, alns, [0], ends=ends)
    with pytest.raises(capi.CdmError, match="cdm error -3.*query index 8"):
        ctx.pileup_profile(db, alns, [0, len(c["seqs"])])
    with pytest.raises(capi.CdmError, match="cdm error -3.*listed twice"):
        ctx.pileup_profile(db, alns, [1, 0, 1])
    counts, reads, _ = ctx.pileup_profile(db, alns, [0])          # (the handles are fine)
    assert reads[0] == 9


def test_a_set_with_the_minus_one_record_is_refused(ctx):
    """a sequence of more than 40 % N scores 0 against itself: cdm_rescore writes its identity record with the coordinates -1, and the
    pile-up refuses the set as cdm_correct does"""
    from carpedeam_amd import synth
    seqs = synth.generate_strings(300, seed=4, mixed=(40, 120))
    rng = np.random.default_rng(5)
    for i in (3, 77, 150, 299):
        s = list(seqs[i])
        for j in rng.choice(len(s), size=len(s) // 2 + 3, replace=False):
            s[j] = "N"
        seqs[i] = "".join(s)
    db = ctx.upload_seqs(seqs)
    alns = ctx.rescore(db, ctx.kmermatch(db))
    _, rec = alns.download()
    assert (rec["q_start"] == -1).any()                 # (the input does reach the case)
    with pytest.raises(capi.CdmError, match="coordinates -1"):
        ctx.pileup_profile(db, alns, [0])


# ------------------------------------------------------------------------------------------------ cdm_seqdb_concat
def check_concat(ctx, a_seqs, b_seqs, a_keys=None, ext_a=1, ext_b=0):
    a = ctx.upload_seqs(a_seqs, keys=a_keys, ext=[0] * len(a_seqs))
    b = ctx.upload_seqs(b_seqs, ext=[1] * len(b_seqs))
    both = ctx.concat(a, b, ext_a, ext_b)
    seqs, keys, ext = both.download()
    want = [s.encode() for s in a_seqs + b_seqs]
    assert seqs == want                                                             # letters: N, lower case and IUPAC codes as they went in
    lens, _, _ = both.meta()
    assert lens.tolist() == [len(s) for s in want]
    assert keys.tolist() == list(range(len(want)))
    assert ext.tolist() == [ext_a] * len(a_seqs) + [ext_b] * len(b_seqs)
    assert both.n == a.n + b.n and both.words == a.words + b.words and both.residues == a.residues + b.residues
    assert both.has_raw == (a.has_raw or b.has_raw)
    return both


def test_concat_plain_and_n(ctx):
    rng = np.random.default_rng(7)
    a = [pc.rand_seq(rng, int(n), 0.05) for n in (400, 16, 17, 1, 32, 33)]
    b = [pc.rand_seq(rng, int(n), 0.05) for n in rng.integers(1, 120, size=40)]
    check_concat(ctx, a, b, a_keys=[3, 5, 8, 13, 21, 34])


def test_concat_with_a_raw_plane_in_one_part_only(ctx):
    rng = np.random.default_rng(8)
    plain = [pc.rand_seq(rng, int(n)) for n in (50, 31, 16)]
    odd = ["acgtNNRYacgtACGTKM", "ACGTTGCAAC", "nnnnACGTacgtwsbdhv" * 3]
    assert check_concat(ctx, plain, odd).has_raw
    assert check_concat(ctx, odd, plain, ext_a=0, ext_b=1).has_raw
    assert check_concat(ctx, odd, odd).has_raw


def test_concat_with_a_single_sequence_of_one_letter(ctx):
    rng = np.random.default_rng(9)
    many = [pc.rand_seq(rng, int(n)) for n in rng.integers(1, 70, size=25)]
    check_concat(ctx, ["G"], many)
    check_concat(ctx, many, ["T"])
    check_concat(ctx, ["N"], ["c"])


def test_the_profile_runs_on_a_concatenated_db(ctx):
    """the layout cdm_seqdb_concat leaves is the one the kernels index: the profile on a concatenated DB equals the model on the joined list"""
    c = pc.raw_plane()
    db = ctx.concat(ctx.upload_seqs(c["seqs"][:2]), ctx.upload_seqs(c["seqs"][2:]), 1, 0)
    c["ext"] = [1, 1, 0, 0, 0]
    c["skip"] = True
    alns = ctx.upload_alns(db, c["off"], c["rec"])
    assert_same(ctx.pileup_profile(db, alns, c["queries"], c["ends"], 0.0, True), model(c))


# ------------------------------------------------------------------------------------------------ pipeline
def test_synth2k_reads_through_kmermatch_and_rescore(ctx):
    """the profile of every query with at least two records against the model on the downloaded records"""
    keyed = gold("synth2k", "reads")
    db = ctx.upload_keyed_seqdb(keyed)
    seqs = [keyed[k][0].rstrip(b"\n").decode() for k in sorted(keyed)]
    alns = ctx.rescore(db, ctx.kmermatch(db))
    off, rec = alns.download()
    queries = [q for q in range(db.n) if off[q + 1] - off[q] >= 2]
    assert len(queries) > 100
    got = ctx.pileup_profile(db, alns, queries, ends=16)
    want = pm.profile(seqs, [0] * db.n, off, rec, queries, 16)
    assert_same(got, want)
    assert want[1].sum() > 1000 and want[0][:, 0, 0].sum() > 1000
