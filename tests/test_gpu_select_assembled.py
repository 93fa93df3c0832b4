"""cdm_seqdb_select_assembled (Ctx.select_assembled): the workflow's selection of the assembled contigs (data/nuclassemble.sh:214-233) on
resident DBs, against a model in Python.  The script's awk filters compare index lengths (sequence + "\\n\\0"): `$3 > $7` is
len(result) > len(source) for the same key, `$3 > thr + 1` is len(result) >= thr."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def ctx():
    from carpedeam_amd import build, capi
    build.build()
    return capi.Ctx(0)


def rand_seq(rng, n, kind=0):
    s = LETTERS[rng.integers(0, 4, n)].copy()
    if kind == 1 and n:        # N
        s[rng.random(n) < 0.15] = ord("N")
    elif kind == 2 and n:      # raw letters: lower case, IUPAC codes
        m = rng.random(n) < 0.2
        s[m] = np.frombuffer(b"acgtnRYKMSWBDHVryk", np.uint8)[rng.integers(0, 18, int(m.sum()))]
    return s.tobytes()


def model(result, source, min_len):
    """result / source: lists of (key, sequence, ext) in key order -> the kept entries of result"""
    src = {k: len(s) for k, s, _ in source}
    return [(k, s, e) for k, s, e in result if k in src and len(s) > src[k] and len(s) >= min_len]


def run(ctx, result, source, min_len):
    up = lambda db: ctx.upload_seqs([s for _, s, _ in db], [k for k, _, _ in db], [e for _, _, e in db])
    r, s = up(result), up(source)
    out = ctx.select_assembled(r, s, min_len)
    seqs, keys, ext = out.download()
    got = [(int(k), bytes(q), int(e)) for q, k, e in zip(seqs, keys, ext)]
    want = model(result, source, min_len)
    assert got == want, (len(got), len(want), [x for x in zip(got, want) if x[0] != x[1]][:2])
    assert out.n == len(want) and out.residues == sum(len(q) for _, q, _ in want)
    return out, got


@pytest.mark.parametrize("n", [1, 2, 7, 64, 65, 200])
def test_random_dbs_against_the_model(ctx, n):
    rng = np.random.default_rng(100 + n)
    keys = np.sort(rng.choice(5 * n + 3, n, replace=False)).tolist()
    source = [(k, rand_seq(rng, int(rng.integers(1, 70)), int(rng.integers(0, 3))), int(rng.integers(0, 2))) for k in keys]
    result = []
    for k, s, _ in source:
        grow = int(rng.integers(-1, 3))                       # shorter by one, equal, longer by one or two
        q = s[:max(len(s) + grow, 1)] if grow <= 0 else s + rand_seq(rng, grow, int(rng.integers(0, 3)))
        result.append((k, q, int(rng.integers(0, 2))))
    for min_len in (0, 1, 20, 35, 1000):
        run(ctx, result, source, min_len)


def test_nothing_kept_and_everything_kept(ctx):
    rng = np.random.default_rng(1)
    source = [(k, rand_seq(rng, 30), 0) for k in range(50)]
    out, got = run(ctx, source, source, 0)                    # equal lengths: not assembled
    assert got == [] and out.n == 0 and out.words == 0 and out.download()[0] == []
    longer = [(k, s + b"A", 1) for k, s, _ in source]
    out, got = run(ctx, longer, source, 0)
    assert len(got) == 50
    out, got = run(ctx, longer, source, 32)                   # every one outgrew its source, none is long enough
    assert got == []
    out, got = run(ctx, longer[:1], source[:1], 31)           # one sequence, kept
    assert len(got) == 1
    out, got = run(ctx, source[:1], source[:1], 0)            # one sequence, dropped
    assert got == []


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_lengths_around_the_word_boundary(ctx, kind):
    """16 letters per code word: 15, 16, 17, 31, 32, 33; equal length is not kept, length + 1 is"""
    rng = np.random.default_rng(7 + kind)
    source, result = [], []
    for i, L in enumerate([15, 16, 17, 31, 32, 33]):
        s = rand_seq(rng, L, kind)
        source += [(2 * i, s, 0), (2 * i + 1, s, 1)]
        result += [(2 * i, rand_seq(rng, L, kind), 1), (2 * i + 1, rand_seq(rng, L + 1, kind), 0)]
    out, got = run(ctx, result, source, 0)
    assert [k for k, _, _ in got] == [1, 3, 5, 7, 9, 11] and [len(q) for _, q, _ in got] == [16, 17, 18, 32, 33, 34]
    assert out.has_raw == (kind == 2)


def test_min_len_at_below_and_above_a_length(ctx):
    rng = np.random.default_rng(3)
    source = [(k, rand_seq(rng, 10), 0) for k in range(3)]
    result = [(0, rand_seq(rng, 47), 0), (1, rand_seq(rng, 48), 0), (2, rand_seq(rng, 49), 0)]
    assert [k for k, _, _ in run(ctx, result, source, 47)[1]] == [0, 1, 2]
    assert [k for k, _, _ in run(ctx, result, source, 48)[1]] == [1, 2]        # exactly at a length: kept (`$3 > thr + 1` on len + 2)
    assert [k for k, _, _ in run(ctx, result, source, 49)[1]] == [2]
    assert [k for k, _, _ in run(ctx, result, source, 50)[1]] == []


def test_letters_and_flags_come_back_byte_for_byte(ctx):
    rng = np.random.default_rng(9)
    source = [(3 * k + 1, rand_seq(rng, 5 + k), k % 2) for k in range(40)]
    result = [(k, rand_seq(rng, len(s) + (i % 3), 1 + i % 2) if i % 5 else b"acgtNNRYacgtnnACGTKMSWBDHV" + s, (i // 2) % 2) for i, (k, s, _) in enumerate(source)]
    out, got = run(ctx, result, source, 0)
    assert any(b"N" in q for _, q, _ in got) and any(q != q.upper() for _, q, _ in got) and any(b"R" in q or b"Y" in q for _, q, _ in got)
    assert {e for _, _, e in got} == {0, 1}                   # wasExtended is the result's, not a constant
    assert out.has_raw


def test_result_keys_are_a_strict_subset_of_the_sources(ctx):
    """the contig phase merges sequences away: the final DB holds fewer keys than the DB the loop started from"""
    rng = np.random.default_rng(11)
    source = [(k, rand_seq(rng, 20), 0) for k in range(0, 200)]
    result = [(k, rand_seq(rng, 20 + (k % 4)), 1) for k in range(0, 200, 7)]
    out, got = run(ctx, result, source, 22)
    assert 0 < len(got) < len(result)
    # a key the source does not hold stands in no line of the script's join: dropped
    result = [(5, rand_seq(rng, 40), 0), (1000, rand_seq(rng, 40), 0)]
    assert [k for k, _, _ in run(ctx, result, source, 0)[1]] == [5]


def test_the_source_may_be_an_index_copy(ctx):
    """what the fused command keeps of the DB it started from: keys and lengths, no letters"""
    rng = np.random.default_rng(13)
    source = [(2 * k, rand_seq(rng, int(rng.integers(1, 40)), k % 3), k % 2) for k in range(130)]
    result = [(k, s + rand_seq(rng, i % 3), 1) for i, (k, s, _) in enumerate(source)]
    full = ctx.upload_seqs([s for _, s, _ in source], [k for k, _, _ in source], [e for _, _, e in source])
    index = ctx.index_copy(full)
    assert index.n == full.n and index.residues == full.residues and index.words == 0
    lens, keys, ext = index.meta()
    assert keys.tolist() == [k for k, _, _ in source] and lens.tolist() == [len(s) for _, s, _ in source] and ext.tolist() == [e for _, _, e in source]
    del full
    r = ctx.upload_seqs([s for _, s, _ in result], [k for k, _, _ in result], [e for _, _, e in result])
    seqs, keys, ext = ctx.select_assembled(r, index, 10).download()
    assert [(int(k), bytes(q), int(e)) for q, k, e in zip(seqs, keys, ext)] == model(result, source, 10)


@pytest.mark.parametrize("keys", [[3, 1, 2], [1, 2, 2], [0, 5, 4, 9]])
def test_a_source_out_of_key_order_is_refused(ctx, keys):
    """shuffled or repeated keys: no sequence DB has them (the index is sorted by key; cdm_seqdb_upload refuses them too), and the look-up
    is a binary search.  Such a DB can only be composed from packed device buffers."""
    import torch
    from carpedeam_amd import capi
    rng = np.random.default_rng(17)
    with pytest.raises(capi.CdmError, match="strictly increasing"):
        ctx.upload_seqs([rand_seq(rng, 20) for _ in keys], keys)
    good = ctx.upload_seqs([rand_seq(rng, 20) for _ in keys])
    n, w = good.n, good.words
    codes, nmask = torch.empty(w, dtype=torch.int32, device="cuda"), torch.empty(w, dtype=torch.int16, device="cuda")
    lens, kk = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    good.copy_packed(codes.data_ptr(), nmask.data_ptr(), lens.data_ptr(), kk.data_ptr())
    ctx.sync()
    kk.copy_(torch.tensor(keys, dtype=torch.int32))
    torch.cuda.synchronize()
    source = ctx.from_packed(codes.data_ptr(), nmask.data_ptr(), lens.data_ptr(), kk.data_ptr(), n, w, 0)
    assert source.meta()[1].tolist() == keys
    result = ctx.upload_seqs([rand_seq(rng, 30)], [1], [0])
    with pytest.raises(capi.CdmError, match="do not ascend strictly"):
        ctx.select_assembled(result, source, 0)
