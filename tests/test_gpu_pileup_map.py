"""cdm_pileup_map on the device against tests/map_model.py: the directed alignment sets of tests/pileupcases.py, directed sets of its own
at the sizes where the mismatch count, the slots, the sort and the gather can go wrong, and the refusals.  Every comparison is between
integers and exact."""
import numpy as np
import pytest

import map_model as mm
import pileupcases as pc
from carpedeam_amd import capi
from pileup_model import unorient

pytestmark = pytest.mark.gpu

COMP = str.maketrans("ACGTN", "TGCAN")


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


def handles(ctx, c):
    db = ctx.upload_seqs(c["seqs"], ext=c["ext"])
    return db, ctx.upload_alns(db, c["off"], c["rec"])


def model(c, queries=None):
    return mm.map_records(c["seqs"], c["ext"], c["off"], c["rec"], c["queries"] if queries is None else queries, c["min_seq_id"], c["skip"])


def check(ctx, c, queries=None, want=None, what="", h=None):
    """the device with and without the records against the model, reads and columns against cdm_pileup_depth; -> the model's results"""
    q = c["queries"] if queries is None else queries
    db, alns = h or handles(ctx, c)
    want_stats, want_recs, want_mism = want or model(c, q)
    plain = ctx.pileup_map(db, alns, q, c["min_seq_id"], c["skip"])
    stats, recs, mism = ctx.pileup_map(db, alns, q, c["min_seq_id"], c["skip"], records=True)
    for got in (plain, stats):
        assert got.dtype == np.uint64 and got.shape == (len(q), 4), what
        assert np.array_equal(got, want_stats), (what, np.argwhere(got != want_stats)[:5].tolist(), got[got != want_stats][:5].tolist(), want_stats[got != want_stats][:5].tolist())
    assert recs.dtype == capi.MAP_DTYPE and recs.shape == want_recs.shape, (what, len(recs), len(want_recs))
    assert np.array_equal(recs, want_recs), (what, [r for r in zip(recs.tolist(), want_recs.tolist()) if r[0] != r[1]][:3])
    assert mism.dtype == np.uint32 and mism.shape == want_mism.shape, (what, len(mism), len(want_mism))
    assert np.array_equal(mism, want_mism), (what, np.flatnonzero(mism != want_mism)[:5].tolist())
    depth = ctx.pileup_depth(db, alns, q, 0, c["min_seq_id"], c["skip"])
    assert np.array_equal(stats[:, :2], depth[:, :2]), what
    return want_stats, want_recs, want_mism


def test_the_binding_agrees_with_the_model_on_the_record():
    assert capi.MAP_DTYPE == mm.MAP_DTYPE and (capi.MAP_REVERSE, capi.MAP_SECONDARY) == (mm.REVERSE, mm.SECONDARY)


@pytest.mark.parametrize("name,make", pc.DIRECTED, ids=[n for n, _ in pc.DIRECTED])
def test_directed_cases(ctx, name, make):
    c = make()
    stats, recs, _ = check(ctx, c, what=name)
    if name == "query_lists":           # the query with only its identity record
        k = c["queries"].index(7)
        assert stats[k].tolist() == [0, 0, 0, 0] and not (recs["query"] == k).any() and (recs["query"] == k - 1).any() and (recs["query"] == k + 1).any()
    if name == "n_columns":
        assert stats[0][2] > 4          # (N columns among the mismatches)


# ------------------------------------------------------------------------------------------------ directed cases of these kernels
PHASES = (15, 16, 17, 31, 32, 33)       # around the 16-base word on both sequences


def phases():
    """a query of 70 letters with two N; one read per (qs, tstart, columns, strand) over PHASES: the query's letters with a mismatch planted
    in the first column, the last column and the last column of a word in turn, an N in the read, an N over the query's N"""
    rng = np.random.default_rng(301)
    q = list(pc.rand_seq(rng, 70))
    q[20] = q[47] = "N"
    seqs = ["".join(q)]
    recs = [pc.identity(seqs, 0)]
    i = 0
    for qs in PHASES:
        for ts in PHASES:
            for n in PHASES:
                for rev in (False, True):
                    body = list(seqs[0][qs:qs + n])
                    plant = []
                    if i % 4 in (1, 3):
                        plant.append(0)
                    if i % 4 in (2, 3):
                        plant.append(n - 1)
                    if i % 3 == 1 and n > 15:
                        plant.append(31 if n > 31 and i % 2 else 15)       # the last column of a 16-column step
                    for col in plant:
                        body[col] = "ACGT"[("ACGT".find(body[col]) + 1) % 4]          # (an N becomes A: still a mismatch, the query's N)
                    if i % 7 == 3:
                        body[7] = "N"
                    if i % 5 == 0 and qs <= 20 < qs + n:
                        body[20 - qs] = "N"
                    oriented = pc.rand_seq(rng, ts) + "".join(body) + pc.rand_seq(rng, i % 3)
                    seqs.append(oriented.translate(COMP)[::-1] if rev else oriented)
                    recs.append(unorient(len(seqs) - 1, qs, qs + n - 1, ts, ts + n - 1, rev, len(oriented)))
                    i += 1
    return pc.case(seqs, {0: recs}, [0])


def test_every_phase_of_the_word_on_both_sequences_and_strands(ctx):
    c = phases()
    stats, recs, mism = check(ctx, c, what="phases")
    assert len(recs) == 2 * len(PHASES) ** 3 and stats[0][3] == len(recs) and (recs["flags"] & mm.REVERSE).sum() == len(recs) // 2
    cols = mism & 0xFFFFFF
    first = mism[recs["mm"][recs["nm"] > 0]] & 0xFFFFFF
    assert (first == 0).any() and (cols == 15).any() and (cols == 31).any() and (recs["nm"] == 0).any()
    last = np.zeros(len(recs), bool)
    for k, r in enumerate(recs):
        last[k] = r["nm"] > 0 and (int(mism[int(r["mm"]) + int(r["nm"]) - 1]) & 0xFFFFFF) == int(r["columns"]) - 1
    assert last.any()
    ref, read = (mism >> 24) & 15, mism >> 28
    assert ((ref == 4) & (read < 4)).any() and ((ref < 4) & (read == 4)).any() and ((ref == 4) & (read == 4)).any()


def test_a_record_of_one_column(ctx):
    seqs = ["ACGTACGTACGTACGTACGT", "T", "GGAGG", "C"]
    recs = [pc.identity(seqs, 0), unorient(1, 19, 19, 0, 0, False, 1), unorient(2, 0, 0, 2, 2, False, 5), unorient(3, 16, 16, 0, 0, False, 1)]
    _, got, mism = check(ctx, pc.case(seqs, {0: recs}, [0]), what="one column")
    assert got["columns"].tolist() == [1, 1, 1] and got["nm"].tolist() == [0, 1, 0] and mism.tolist() == [0 | 0 << 24 | 1 << 28]


@pytest.mark.parametrize("extra", [0, 1])
def test_a_chunk_of_records_and_one_more(ctx, extra):
    n = capi.pileup_chunk_records() + extra
    stats, recs, _ = check(ctx, pc.depth(n), what="chunk + %d" % extra)
    assert len(recs) == n


@pytest.mark.parametrize("n", [8191, 8192, 8193, 20000])
def test_around_the_radix_tile_and_beyond(ctx, n):
    stats, recs, _ = check(ctx, pc.depth(n), what="%d records" % n)
    assert len(recs) == n and stats[0][0] == n and (np.diff(recs["pos"].astype(np.int64)) >= 0).all()


def test_all_records_at_one_position_keep_the_order_of_the_set(ctx):
    rng = np.random.default_rng(302)
    seqs = [pc.rand_seq(rng, 90)] + [pc.rand_seq(rng, int(n)) for n in rng.integers(2, 60, size=9)]
    recs = [pc.identity(seqs, 0)]
    for i in range(300):
        t = 1 + i % 9
        n = int(rng.integers(2, len(seqs[t]) + 1))
        ds = int(rng.integers(0, len(seqs[t]) - n + 1))
        recs.append(unorient(t, 10, 10 + n - 1, ds, ds + n - 1, bool(i % 2), len(seqs[t])))
    c = pc.case(seqs, {0: recs}, [0])
    _, got, _ = check(ctx, c, what="one pos")
    assert (got["pos"] == 10).all() and got["target"].tolist() == [int(r[0]) for r in recs[1:]] and (got["flags"] & mm.SECONDARY == 0).sum() == 9


def test_positions_descending_in_the_set(ctx):
    rng = np.random.default_rng(303)
    seqs = [pc.rand_seq(rng, 150), pc.rand_seq(rng, 20), pc.rand_seq(rng, 20)]
    recs = [pc.identity(seqs, 0)] + [unorient(1 + qs % 2, qs, qs + 19, 0, 19, qs % 3 == 0, 20) for qs in range(130, -1, -1)]
    _, got, _ = check(ctx, pc.case(seqs, {0: recs}, [0]), what="descending")
    assert got["pos"].tolist() == list(range(131))


def test_positions_in_every_digit_of_the_sort_key(ctx):
    """one query of 270 000 letters with records around 2^9 and 2^18 and spread between, descending in the set: every 9-bit digit of the
    position bits of the sort key decides somewhere"""
    rng = np.random.default_rng(305)
    n = 270_000
    seqs = [pc.rand_seq(rng, n, 0.001), pc.rand_seq(rng, 30), pc.rand_seq(rng, 17)]
    at = sorted(set([0, 510, 511, 512, 513, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, n - 30] + [int(x) for x in rng.integers(0, n - 30, size=600)]), reverse=True)
    recs = [pc.identity(seqs, 0)]
    for i, qs in enumerate(at):
        recs.append(unorient(1, qs, qs + 29, 0, 29, bool(i % 2), 30))
        if i % 3 == 0:
            recs.append(unorient(2, qs, qs + 16, 0, 16, False, 17))
    _, got, _ = check(ctx, pc.case(seqs, {0: recs}, [0]), what="long query")
    pos = got["pos"].astype(np.int64)
    assert (np.diff(pos) >= 0).all() and pos[-1] == n - 30 and (pos >> 18).max() == 1 and ((pos >> 9) & 511).max() == 511


@pytest.mark.parametrize("m", [257, 513, 4097])
def test_query_counts_around_the_digits_of_the_sort_key(ctx, m):
    """m listed queries, one more than a power of two: the last query's index needs one more key bit (and at 513 and 4097 one more radix
    pass) than the others"""
    rng = np.random.default_rng(306)
    seqs = [pc.rand_seq(rng, 24) for _ in range(m)] + [pc.rand_seq(rng, 12) for _ in range(3)]
    per = {}
    for q in range(m):
        per[q] = [pc.identity(seqs, q), unorient(m + q % 3, (q * 5) % 13, (q * 5) % 13 + 11, 0, 11, bool(q % 2), 12)]
        if q % 2:
            per[q].append(unorient(m + (q + 1) % 3, (q * 3) % 13, (q * 3) % 13 + 11, 0, 11, False, 12))
    c = pc.case(seqs, per, list(range(m - 1, -1, -1)))
    stats, got, _ = check(ctx, c, what="%d queries" % m)
    assert (np.diff(got["query"].astype(np.int64)) >= 0).all() and got["query"][-1] == m - 1 and stats[:, 3].sum() == 3


def test_query_orders_and_a_query_without_reads_between_two_with(ctx):
    c = pc.query_lists()
    h = handles(ctx, c)
    for q in ([29, 17, 7, 4, 3], [29, 7, 3], [3, 7, 29], [7], list(range(29, -1, -1))):
        stats, recs, _ = check(ctx, c, queries=q, what=str(q), h=h)
        k = q.index(7)
        assert stats[k].tolist() == [0, 0, 0, 0] and (np.diff(recs["query"].astype(np.int64)) >= 0).all()


def test_a_read_on_three_queries_of_which_one_is_not_listed(ctx):
    """the read's longest record is on the unlisted query: of the other two the longer is the primary; with all three listed it is not"""
    rng = np.random.default_rng(304)
    seqs = [pc.rand_seq(rng, 60) for _ in range(3)] + [pc.rand_seq(rng, 40)]
    per = {q: [pc.identity(seqs, q)] for q in range(3)}
    per[0].append(unorient(3, 5, 24, 0, 19, False, 40))
    per[1].append(unorient(3, 0, 39, 0, 39, True, 40))
    per[2].append(unorient(3, 30, 54, 10, 34, False, 40))
    c = pc.case(seqs, per, [2, 0])
    h = handles(ctx, c)
    _, recs, _ = check(ctx, c, what="two of three", h=h)
    assert [(int(r["query"]), int(r["flags"])) for r in recs] == [(0, 0), (1, mm.SECONDARY)]
    _, recs, _ = check(ctx, c, queries=[2, 1, 0], what="all three", h=h)
    assert [(int(r["query"]), int(r["flags"])) for r in recs] == [(0, mm.SECONDARY), (1, mm.REVERSE), (2, mm.SECONDARY)]


def test_small_chunks_slices_and_batches(ctx, monkeypatch):
    """the same results when a query's records are cut into items of 3, the items into launches of 5 and the listed queries into batches
    of at most 7 records (most queries go alone): the primary is still chosen over the whole call, the records come in listed order"""
    c = pc.query_lists()
    q = [17, 3, 29, 7, 4, 0, 1, 2]
    want = model(c, q)
    d = pc.depth(129)
    want_d = model(d)
    before = capi.pileup_chunk_records()
    monkeypatch.setenv("CDM_PILEUP_CHUNK", "3")
    monkeypatch.setenv("CDM_LAUNCH_SLICE", "5")
    monkeypatch.setenv("CDM_MAP_BATCH", "7")
    assert capi.pileup_chunk_records() == 3
    check(ctx, c, queries=q, want=want, what="query_lists, small switches")
    check(ctx, d, want=want_d, what="depth_129, small switches")
    monkeypatch.delenv("CDM_PILEUP_CHUNK")
    monkeypatch.delenv("CDM_LAUNCH_SLICE")
    monkeypatch.delenv("CDM_MAP_BATCH")
    assert capi.pileup_chunk_records() == before
    check(ctx, c, queries=q, want=want, what="query_lists, switches restored")
    assert len(set(want[1]["query"].tolist())) >= 6 and (want[1]["flags"] & mm.SECONDARY).any()


def test_refusals(ctx):
    c = pc.one_query_of_40()
    db, alns = handles(ctx, c)
    for records in (False, True):
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_map: query index 8"):
            ctx.pileup_map(db, alns, [0, len(c["seqs"])], records=records)
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_map: query index 1 is listed twice"):
            ctx.pileup_map(db, alns, [1, 0, 1], records=records)
        other = ctx.upload_seqs(c["seqs"][:3])
        with pytest.raises(capi.CdmError, match="cdm error -3.*cdm_pileup_map: alignment CSR has 8 queries, DB has 3"):
            ctx.pileup_map(other, alns, [0], records=records)
    check(ctx, c, what="the handles are fine")


def test_a_set_with_the_minus_one_record_is_refused(ctx):
    """a sequence of more than 40 % N scores 0 against itself: cdm_rescore writes its identity record with the coordinates -1, and the
    call refuses the set as the depth does"""
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
    with pytest.raises(capi.CdmError, match="cdm_pileup_map.*coordinates -1"):
        ctx.pileup_map(db, alns, [0], records=True)


def test_the_empty_query_list_and_the_time(ctx):
    c = pc.query_lists()
    db, alns = handles(ctx, c)
    stats = ctx.pileup_map(db, alns, [])
    assert stats.shape == (0, 4) and stats.dtype == np.uint64
    stats, recs, mism = ctx.pileup_map(db, alns, [], records=True)
    assert stats.shape == (0, 4) and recs.shape == (0,) and recs.dtype == capi.MAP_DTYPE and mism.shape == (0,)
    stats, recs, mism = ctx.pileup_map(db, alns, [7], records=True)          # (the binding asserts: no records, NULL arrays)
    assert stats.tolist() == [[0, 0, 0, 0]] and len(recs) == 0 and len(mism) == 0
    ctx.pileup_map(db, alns, c["queries"], records=True)
    assert ctx.map_kernel_ms > 0
