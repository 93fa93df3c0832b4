"""cdm_rescore's one-pass kernel (k_rescore scores a tile of hits, compacts the survivors and writes the per-query offsets) against
the two-pass form it replaced (CDM_RESCORE=twopass), which tests/test_gpu_rescore.py holds to the goldens and the oracle: `off`, `rec`
(all eight fields, bit for bit), `ryMism`, `count` and `undefinedRecords` must be identical on hit sets placed on the kernel's tile
boundaries.  The switch is read from the library's snapshot of the environment, so each form runs in a fresh child process: this
file, run as a script, computes every case and writes the results to one .npz.

The kernel is a loop: a block takes tiles by ticket, and writes a tile after it has scored its next one (two record buffers and two
ticket slots that alternate, a last write behind the loop).  With the grid a device gives it every set here is one tile per block, so
the one-pass form also runs with CDM_RESCORE_BLOCKS=1 and =3: one block takes every tile in turn, three blocks share them, and the
nine-tile set puts a tile without survivors and the tile-crossing queries into a block's later iterations.

Valid and invalid hits by construction: a hit between two copies of one read (diagonal 0) passes every gate, a hit between two reads
that share fewer than 60 % of their first letters fails them, kmermatch's own hits are mostly valid."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

N_BASE, N_COPIES, COPY_OF = 2000, 320, 7        # reads of 60-150 bp, then copies of read COPY_OF: queries N_BASE.. are the copies
HEAVY = [3, 77, 150, 299]                        # the identity case: reads with more than half of their letters N


def reads():
    from carpedeam_amd import synth
    base = synth.generate_strings(N_BASE, seed=21, mixed=(60, 150))
    return base + [base[COPY_OF]] * N_COPIES


def identity_case_reads():
    """the input of test_gpu_rescore.py::test_identity_record_of_a_sequence_that_scores_zero_against_itself"""
    from carpedeam_amd import synth
    seqs = synth.generate_strings(300, seed=4, mixed=(40, 120))
    rng = np.random.default_rng(5)
    for i in HEAVY:
        s = list(seqs[i])
        for j in rng.choice(len(s), size=len(s) // 2 + 3, replace=False):
            s[j] = "N"
        seqs[i] = "".join(s)
    return seqs


class Builder:
    """hit sets over the reads(): lists of (query, target, score, diagonal) in query order"""

    def __init__(self, seqs, koff, krec):
        self.seqs, self.koff, self.krec, self.n = seqs, koff, krec, len(seqs)

    def bad(self, q, i):
        """the i-th injected hit of query q: an unrelated base read on diagonal 0 (fewer than 60 % of the compared letters agree)"""
        t = (q + 611 + 37 * i) % N_BASE
        while True:
            a, b = self.seqs[q], self.seqs[t]
            m = min(len(a), len(b))
            if t != q and t != COPY_OF and sum(x == y for x, y in zip(a[:m], b[:m])) < 0.6 * m:
                return (q, t, 1, 0)
            t = (t + 1) % N_BASE

    def real(self, q0, count, every=20):
        """`count` hits of kmermatch for the queries from q0 on (the last query's list may be cut), every `every`-th one replaced by
        an injected hit -> (hits, the first query not used)"""
        out, q = [], q0
        while len(out) < count:
            assert q < N_BASE
            for k in range(int(self.koff[q]), int(self.koff[q + 1])):
                if len(out) == count:
                    break
                r = self.krec[k]
                out.append(self.bad(q, k) if len(out) % every == every - 1 else (q, int(r["target"]), int(r["score"]), int(r["diagonal"])))
            q += 1
        return out, q

    def copies(self, q, count, bad_every=0):
        """`count` hits of the copy read q: other copies (valid, distinct neighbours), every bad_every-th one an injected hit"""
        out = []
        for i in range(count):
            if bad_every and i % bad_every == bad_every - 1:
                out.append(self.bad(q, i))
            else:
                out.append((q, N_BASE + (q - N_BASE + 1 + i % (N_COPIES - 1)) % N_COPIES, 1, 0))
        return out

    def csr(self, hits):
        from carpedeam_amd import capi
        qs = np.array([h[0] for h in hits], np.int64)
        assert np.all(np.diff(qs) >= 0)
        off = np.zeros(self.n + 1, np.uint64)
        off[1:] = np.cumsum(np.bincount(qs, minlength=self.n)) if len(hits) else 0
        rec = np.array([h[1:] for h in hits], capi.HIT_DTYPE) if hits else np.zeros(0, capi.HIT_DTYPE)
        return off, rec


def build_cases(b, T):
    cases, marks = {}, {}
    for name, nh in (("n0", 0), ("n1", 1), ("nT-1", T - 1), ("nT", T), ("nT+1", T + 1)):
        cases[name] = b.real(0, nh)[0]
    # 3T + 1 hits, the second tile without a valid hit: the chain passes a zero count
    front, q = b.real(0, T)
    mid = [b.bad(q + k, i) for k, cnt in enumerate((T // 2, T // 4, T - T // 2 - T // 4)) for i in range(cnt)]
    cases["3T+1_middle_tile_invalid"] = front + mid + b.real(q + 3, T + 1)[0]
    # queries without hits: 0..2 in front, one alone, five in a row, the copies at the end; one query with invalid hits only
    h1, q1 = b.real(3, 40)
    h2, q2 = b.real(q1 + 1, T)
    h3, q3 = b.real(q2 + 6, 60)
    cases["empty_queries"] = h1 + h2 + [b.bad(q2 + 5, i) for i in range(7)] + h3 + b.real(q3 + 2, T - 63)[0]
    marks["empty_queries"] = np.array([q1, q2, q2 + 5], np.int64)       # the lone empty query, the first of five, the all-invalid one
    cases["all_invalid"] = [b.bad(q, i) for q in range(10, 10 + (2 * T + 5 + 6) // 7) for i in range(7)][:2 * T + 5]
    cases["eighth_invalid"] = b.real(0, 2 * T + 100, every=3)[0]
    # one query across a tile boundary: hits T - 3 .. T + 4
    front, _ = b.real(0, T - 3)
    cases["straddle"] = front + b.copies(N_BASE, 8, bad_every=3) + b.copies(N_BASE + 5, 4)
    # one query with T + 80 > 256 hits that begins in the first tile and ends in the third
    front, _ = b.real(0, T - 40)
    cases["deep_query"] = front + b.copies(N_BASE + 2, T + 80, bad_every=3) + b.copies(N_BASE + 9, 3)
    # nine tiles and five hits for the grids of one and three blocks: tile 4 without survivors, a query across tiles 5 | 6, one
    # across 6, 7 and 8, a last tile of five hits
    front, q = b.real(0, 4 * T)
    mid = [b.bad(q + k, i) for k, cnt in enumerate((T // 2, T // 4, T - T // 2 - T // 4)) for i in range(cnt)]
    cases["nine_tiles"] = (front + mid + b.real(q + 3, T - 3)[0] + b.copies(N_BASE, 8, bad_every=3) + b.copies(N_BASE + 2, 2 * T + 80, bad_every=3)
                           + b.copies(N_BASE + 9, T - 80))
    return cases, marks


def child(out_path):
    sys.path.insert(0, ROOT)
    from carpedeam_amd import capi
    ctx = capi.Ctx(0)
    T = ctx.rescore_tile()
    res = {"T": np.int64(T)}

    def run(name, db, hits, hoff, hrec):
        alns = ctx.rescore(db, hits)
        off, rec = alns.download()
        res.update({name + "/off": off, name + "/rec": rec, name + "/ry": alns.download_ry(), name + "/count": np.int64(alns.count),
                    name + "/undef": np.int64(alns.undefined_records), name + "/hoff": hoff, name + "/hrec": hrec})

    seqs = reads()
    db = ctx.upload_seqs(seqs)
    koff, krec = ctx.kmermatch(db).download()
    b = Builder(seqs, koff, krec)
    assert np.all(np.diff(koff.astype(np.int64))[:N_BASE] > 0)      # (every read is at least its own hit: Builder.real leaves no query out)
    cases, marks = build_cases(b, T)
    res.update({name + "/marks": m for name, m in marks.items()})
    for name, hits in cases.items():
        hoff, hrec = b.csr(hits)
        run(name, db, ctx.upload_hits(db, hoff, hrec), hoff, hrec)
    db = ctx.upload_seqs(identity_case_reads())
    hits = ctx.kmermatch(db)
    run("identity", db, hits, *hits.download())
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """{form: results of every case}, each form computed by one fresh process"""
    d = tmp_path_factory.mktemp("onepass")
    got = {}
    for form, switches in FORMS.items():
        env = {k: v for k, v in os.environ.items() if k not in ("CDM_RESCORE", "CDM_RESCORE_BLOCKS")}
        env.update(switches)
        out = str(d / (form + ".npz"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True)
        assert r.returncode == 0, (form, r.stdout[-2000:], r.stderr[-4000:])
        got[form] = dict(np.load(out))
    return got


FORMS = {"onepass": {}, "twopass": {"CDM_RESCORE": "twopass"}, "onepass_1_block": {"CDM_RESCORE_BLOCKS": "1"}, "onepass_3_blocks": {"CDM_RESCORE_BLOCKS": "3"}}
CASES = ["nine_tiles", "n0", "n1", "nT-1", "nT", "nT+1", "3T+1_middle_tile_invalid", "empty_queries", "all_invalid", "eighth_invalid", "straddle", "deep_query", "identity"]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("form", [f for f in FORMS if f != "twopass"])
def test_one_pass_equals_two_pass(both, form, name):
    a, b = both[form], both["twopass"]
    assert np.array_equal(a[name + "/hoff"], b[name + "/hoff"]) and a[name + "/hrec"].tobytes() == b[name + "/hrec"].tobytes()      # same input
    assert int(a[name + "/count"]) == int(b[name + "/count"])
    assert int(a[name + "/undef"]) == int(b[name + "/undef"])
    assert np.array_equal(a[name + "/off"], b[name + "/off"])
    assert a[name + "/rec"].dtype.itemsize == 32 and a[name + "/rec"].tobytes() == b[name + "/rec"].tobytes()
    assert np.array_equal(a[name + "/ry"], b[name + "/ry"])
    assert int(a[name + "/off"][-1]) == int(a[name + "/count"]) == len(a[name + "/rec"])


def per_query(res, name):
    return np.diff(res[name + "/hoff"].astype(np.int64)), np.diff(res[name + "/off"].astype(np.int64))


def test_the_cases_reach_what_they_are_for(both):
    """read from the two-pass results and the inputs: the sets do hold the tile counts, the empty and the invalid queries, the two
    sides of the allocation rule and the tile-crossing queries that their names promise"""
    r = both["twopass"]
    T = int(r["T"])
    assert T == int(both["onepass"]["T"]) and T % 256 == 0
    for name, nh in (("n0", 0), ("n1", 1), ("nT-1", T - 1), ("nT", T), ("nT+1", T + 1), ("3T+1_middle_tile_invalid", 3 * T + 1)):
        assert len(r[name + "/hrec"]) == nh, name
    assert int(r["n0/count"]) == 0 and not r["n0/off"].any()
    # sizes that keep the large arrays (at most an eighth unused), and sets that take the copy into arrays of their own size
    for name in ("nT-1", "nT", "nT+1", "straddle"):
        nh = len(r[name + "/hrec"])
        assert nh - int(r[name + "/count"]) <= nh // 8, name
    for name in ("3T+1_middle_tile_invalid", "all_invalid", "eighth_invalid"):
        nh = len(r[name + "/hrec"])
        assert nh - int(r[name + "/count"]) > nh // 8, name
    assert int(r["all_invalid/count"]) == 0 and not r["all_invalid/off"].any()
    assert int(r["eighth_invalid/count"]) > 0
    # the second tile of 3T + 1: no survivor among the hits T .. 2T - 1, survivors on both sides
    hq, aq = per_query(r, "3T+1_middle_tile_invalid")
    hoff = r["3T+1_middle_tile_invalid/hoff"].astype(np.int64)
    inside = (hoff[:-1] >= T) & (hoff[1:] <= 2 * T) & (hq > 0)
    assert hq[inside].sum() == T and aq[inside].sum() == 0
    assert aq[hoff[1:] <= T].sum() > 0 and aq[hoff[:-1] >= 2 * T].sum() > 0
    # queries without hits: the first three, one alone, five in a row, the last ones; one query has hits and no survivor
    hq, aq = per_query(r, "empty_queries")
    lone, run, bad = (int(x) for x in r["empty_queries/marks"])
    assert not hq[:3].any() and hq[3] > 0 and hq[lone - 1] > 0 and hq[lone] == 0 and hq[lone + 1] > 0
    assert hq[run - 1] > 0 and not hq[run:run + 5].any() and bad == run + 5 and not hq[N_BASE:].any()
    assert hq[bad] == 7 and aq[bad] == 0 and np.all(aq[hq == 0] == 0) and aq.sum() > 0
    # the tile-crossing queries
    hoff = r["straddle/hoff"].astype(np.int64)
    assert hoff[N_BASE] == T - 3 and hoff[N_BASE + 1] == T + 5
    hoff = r["deep_query/hoff"].astype(np.int64)
    q = N_BASE + 2
    assert hoff[q] < T and hoff[q + 1] > 2 * T and hoff[q + 1] - hoff[q] > 256
    # nine tiles: 9T + 5 hits, none of the hits 4T .. 5T - 1 survives, a query over the hits 6T - 3 .. 6T + 4, one from tile 6 into tile 8
    hq, aq = per_query(r, "nine_tiles")
    hoff = r["nine_tiles/hoff"].astype(np.int64)
    assert hoff[-1] == 9 * T + 5
    inside = (hoff[:-1] >= 4 * T) & (hoff[1:] <= 5 * T) & (hq > 0)
    assert hq[inside].sum() == T and aq[inside].sum() == 0 and aq[hoff[1:] <= 4 * T].sum() > 0
    assert hoff[N_BASE] == 6 * T - 3 and hoff[N_BASE + 1] == 6 * T + 5 and aq[N_BASE] > 0
    assert 6 * T < hoff[q] < 7 * T and hoff[q + 1] > 8 * T and aq[q] > T


def test_order_inside_a_deep_query(both):
    """a query's records keep their hit order: the copies among the hits of the deep query, in the order of the hits"""
    for form in FORMS:
        r = both[form]
        q = N_BASE + 2
        for name in ("deep_query", "nine_tiles"):
            h = r[name + "/hrec"][int(r[name + "/hoff"][q]):int(r[name + "/hoff"][q + 1])]
            want = h["target"][h["target"] >= N_BASE]
            assert 0 < len(want) < len(h)
            got = r[name + "/rec"][int(r[name + "/off"][q]):int(r[name + "/off"][q + 1])]
            assert np.array_equal(got["target"], want), (form, name)


def test_identity_records_with_the_coordinates_minus_one(both):
    for form in ("onepass", "twopass"):
        r = both[form]
        assert int(r["identity/undef"]) == len(HEAVY)
        for q in HEAVY:
            recs = r["identity/rec"][int(r["identity/off"][q]):int(r["identity/off"][q + 1])]
            own = recs[recs["target"] == q]
            assert len(own) == 1 and own[0]["q_start"] == -1 and own[0]["q_end"] == -1 and own[0]["db_start"] == -1 and own[0]["db_end"] == -1, (form, q)
        assert np.all(r["identity/ry"][(r["identity/rec"]["q_start"] == -1) & (r["identity/rec"]["q_end"] == -1)] == 0xFFFF)


if __name__ == "__main__":
    child(sys.argv[1])
