"""Directed corpora for the grouping kernel of the slot layout (kmer_group.h k_bucket_groups<LayoutSlot, u32>, bucket.h's 32-bit
exchange network): every case's prefilter output under CDM_KMER_LAYOUT=slot is compared with the 12-byte layout's and with the oracle's.

What the corpora are built around (a k-mer's index has its first letter in the top bits, A,C,T,G = 0..3, and the smaller of the
k-mer and its reverse complement is kept; 27 of the 40 bits are sorted globally, so a bucket is the k-mers that agree in their first
13 letters and the top bit of the 14th):
- a random 20-mer X that m reads carry once each, a bucket of exactly m tuples, one run (the windows next to X scatter: see
  shared_kmer below); three 20-mers that differ in their last letter: one bucket of three runs.
  The library's CDM_BUCKET_STATS line (buckets left to the caller, their tuples) checks that the corpus is what it claims to be;
- A^20, the smallest k-mer there is: its run is the first of the array (the reference's repIsReverse quirk), in the first wave's window;
- a 20-mer a read carries twice or three times (--ignore-multi-kmer 0: the extractor keeps them), as the run's representative and as
  a later member;
- neighbours in slot order: the last k-mer position of read i and the first of read i + 1, identical neighbours, a read next to its
  reverse complement, and copies of a read whose whole-sequence hash tuple stays in slot 0 (tests/golden/extract_uniform).
"""
import os

import numpy as np
import pytest

from carpedeam_amd import capi, mmdb
from gpuutil import diff_keys, run_oracle
from stageflags import K_FLAGS

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extract_uniform")
K = 20
FORCED = ({"CDM_FORCE_WIDE_KEY": "1"}, {"CDM_REC_LIMIT": "2"})


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def background(rng, n, L):
    """n reads of a random genome at about 8 x coverage, both strands: ordinary buckets of a few tuples"""
    G = max(2 * L, n * L // 8)
    genome = rand_seq(rng, G + L)
    out = []
    for _ in range(n):
        st = int(rng.integers(0, G))
        s = genome[st:st + L]
        out.append(revcomp(s) if rng.random() < 0.5 else s)
    return out


def around(rng, motif, L, pos=None, rc=False):
    """a random read of L letters with `motif` at `pos` (random if None), or its reverse complement (the poly-A motifs bring the letters
    that end their run of A along)"""
    pos = int(rng.integers(0, L - len(motif) + 1)) if pos is None else pos
    left, right = rand_seq(rng, pos), rand_seq(rng, L - pos - len(motif))
    s = left + motif + right
    assert len(s) == L
    return revcomp(s) if rc else s


def text(ctx, keyed, par):
    db = ctx.upload_keyed_seqdb(keyed)
    _, keys, _ = db.meta()
    off, rec = ctx.kmermatch(db, par).download()
    return {k: (v, 0) for k, v in capi.hits_to_text(off, rec, keys).items()}


def check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, ignore_multi=1, caps=(), forced=FORCED):
    """slot layout == 12-byte layout == oracle; the slot layout again with every capacity of `caps` and every forced variant"""
    assert len(set(len(s) for s in seqs)) == 1
    t = lambda s: str(tmp_path / s)
    mmdb.write_seqdb(t("in"), seqs)
    flags = list(K_FLAGS)
    flags[flags.index("--ignore-multi-kmer") + 1] = str(ignore_multi)
    run_oracle(oracle_bin, "kmermatcher", t("in"), t("pref"), *flags, "--threads", "4")
    want = {k: (v[0], 0) for k, v in mmdb.read_db(t("pref")).items()}
    keyed = mmdb.read_db(t("in"))
    par = capi.KmerParams(K, 200, 0.2, 67, ignore_multi, 0, 1, 0.0)
    runs = [{"CDM_KMER_LAYOUT": "packed"}, {"CDM_KMER_LAYOUT": "slot"}]
    runs += [{"CDM_KMER_LAYOUT": "slot", "CDM_BUCKET_CAP": str(c)} for c in caps]
    runs += [dict(e, CDM_KMER_LAYOUT="slot") for e in forced]
    for env in runs:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        bad = diff_keys(text(ctx, keyed, par), want)
        for k in env:
            monkeypatch.delenv(k)
        assert not bad, (env, bad[:8])
    return keyed, par


def big_buckets(ctx, capfd, monkeypatch, keyed, par, cap):
    """(buckets, tuples) the grouping kernel of the slot layout left to the caller, from the library's CDM_BUCKET_STATS line"""
    env = {"CDM_KMER_LAYOUT": "slot", "CDM_BUCKET_STATS": "1"}
    if cap is not None:
        env["CDM_BUCKET_CAP"] = str(cap)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    text(ctx, keyed, par)
    err = capfd.readouterr().err
    for k in env:
        monkeypatch.delenv(k)
    lines = [x for x in err.splitlines() if x.startswith("kmermatch sort 1:")]
    assert "kmermatch extraction" in err, "no statistics on stderr"
    if not lines:              # (the line is written when there is such a bucket)
        return 0, 0
    words = lines[-1].split(":")[-1].split()
    return int(words[0]), int(words[3])


# ---- buckets of a chosen size
# The 20-mer X = A G^6 ...... C^6 z (z not T) is the smaller of itself and its reverse complement.  The windows next to it share most of
# their letters from read to read; with the six letters in front of X drawn from A, C, T and the six behind it from A, T, G they are kept
# on the strand whose first letter is one of those flank letters (it is below the G / the complement of C on the other strand), so they
# scatter over buckets of about a third of the carriers and less, and the bucket of X holds the carriers' tuples alone.
def shared_kmer(rng, last="A"):
    assert last in "ACG"
    return "A" + "G" * 6 + rand_seq(rng, 6) + "C" * 6 + last


def pick(rng, letters, n):
    return "".join(letters[i] for i in rng.integers(0, len(letters), n))


def carriers(rng, X, n, L):
    """n reads that carry the 20-mer X once, at a random position, on either strand"""
    out = []
    for _ in range(n):
        pos = int(rng.integers(0, L - K + 1))
        room = L - pos - K
        left = rand_seq(rng, max(0, pos - 6)) + pick(rng, "ACT", min(6, pos))
        right = pick(rng, "ATG", min(6, room)) + rand_seq(rng, max(0, room - 6))
        s = left + X + right
        assert len(s) == L
        out.append(revcomp(s) if rng.random() < 0.5 else s)
    return out


@pytest.mark.parametrize("m", [1, 63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_every_network_size(ctx, oracle_bin, tmp_path, monkeypatch, capfd, m):
    """one bucket of m tuples among buckets of a few.  Without a capacity it is part of a group of up to 256 (the 256-word network; 257
    goes to the caller's list); with the capacity m it fills a group by itself on the network of 64, 128 or 256 words that m needs, with
    m - 1 it is left to the caller, and with 64 / 128 every group of the corpus takes the small networks"""
    rng = np.random.default_rng(1000 + m)
    motif = carriers(rng, shared_kmer(rng), m, 100)
    bg = background(rng, 400, 100)
    seqs = motif[:1] + bg[:200] + motif[1:] + bg[200:]
    caps = sorted(set(c for c in (m, m - 1, 64, 128) if 1 <= c <= 256))
    keyed, par = check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, caps=caps)
    # the corpus is what it claims to be: the bucket is finished on chip at the capacity m and is the only one left to the caller at m - 1
    if m >= 63:
        assert big_buckets(ctx, capfd, monkeypatch, keyed, par, min(m, 256)) == ((0, 0) if m <= 256 else (1, m))
        assert big_buckets(ctx, capfd, monkeypatch, keyed, par, min(m - 1, 256)) == (1, m)


@pytest.mark.parametrize("n1,n2,n3", [(64, 128, 64), (40, 128, 88), (32, 64, 32), (33, 63, 30), (64, 0, 0), (100, 0, 0)])
def test_runs_and_rows_of_64_sorted_positions(ctx, oracle_bin, tmp_path, monkeypatch, capfd, n1, n2, n3):
    """three k-mers that differ in their last letter: one bucket of n1 + n2 + n3 tuples that fills the capacity, so it is a group of
    its own and its runs end at the sorted positions n1, n1 + n2 and n1 + n2 + n3 - (64, 128, 64): exactly on the rows 64 and 192 of the
    256-word network; (40, 128, 88): the middle run crosses two rows; (32, 64, 32) and (33, 63, 30): the 128-word network; (64) a run that
    is a whole row and a whole group; (100): one that crosses a row and ends inside the next"""
    rng = np.random.default_rng(7 * n1 + n2)
    X = shared_kmer(rng)
    motif = []
    for last, n in zip("ACG", (n1, n2, n3)):           # (ascending: A, C, T, G = 0..3)
        motif += carriers(rng, X[:-1] + last, n, 100)
    order = rng.permutation(len(motif))
    seqs = background(rng, 150, 100) + [motif[i] for i in order] + background(rng, 150, 100)
    total = n1 + n2 + n3
    keyed, par = check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, caps=(total, 256))
    assert big_buckets(ctx, capfd, monkeypatch, keyed, par, total) == (0, 0)
    assert big_buckets(ctx, capfd, monkeypatch, keyed, par, total - 1) == (1, total)


# ---- the first run of the array
def first_bucket_reads(rng, L, nP, nQ, nQ2, first_rc=False, mix=True):
    """reads around C A^20 C (they carry A^20, A^19 C and C A^19), G A^19 C and C A^19 G; the first one on the strand asked for"""
    reads = [around(rng, "C" + "A" * 20 + "C", L, rc=(first_rc if i == 0 else (mix and rng.random() < 0.5))) for i in range(nP)]
    reads += [around(rng, "G" + "A" * 19 + "C", L, rc=(mix and rng.random() < 0.5)) for _ in range(nQ)]
    reads += [around(rng, "C" + "A" * 19 + "G", L, rc=(mix and rng.random() < 0.5)) for _ in range(nQ2)]
    return reads


@pytest.mark.parametrize("first_rc", [False, True])
def test_first_run_of_the_array(ctx, oracle_bin, tmp_path, monkeypatch, first_rc):
    """A^20 is the smallest k-mer there is: its run is the first of the array, in the first wave's window.  Its representative - the read
    with the smallest id - carries it on the forward strand, or as T^20 (the reference keeps repIsReverse = false for this one run)"""
    rng = np.random.default_rng(41 + first_rc)
    motif = first_bucket_reads(rng, 100, 9, 5, 4, first_rc=first_rc)
    seqs = motif[:1] + background(rng, 350, 100) + motif[1:]
    check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, caps=(64, 23))
    # ... and with no other read on the representative's strand / only such reads
    motif = first_bucket_reads(rng, 100, 6, 0, 0, first_rc=first_rc, mix=False)
    check(ctx, oracle_bin, tmp_path, monkeypatch, motif[:1] + background(rng, 200, 100) + motif[1:], forced=())


# ---- a k-mer twice and three times in one read
def tandem_read(rng, X, times, L):
    gap = (L - times * K) // (times + 1)
    s = ""
    for _ in range(times):
        s += rand_seq(rng, gap) + X
    return s + rand_seq(rng, L - len(s))


def test_tandem_repeats(ctx, oracle_bin, tmp_path, monkeypatch):
    """--ignore-multi-kmer 0: a read keeps a k-mer it carries two or three times.  As the representative of the run (the smallest id:
    its smaller position wins, on the forward strand or - the reverse complement of the 20-mer in the read - counted from the other end),
    as a later member, as the only two tuples of a run, and with the 20-mer on both strands of one read"""
    rng = np.random.default_rng(77)
    L = 100
    head, tail = [], []
    for variant in range(2):                     # the 20-mer as drawn / reverse-complemented: one is the canonical strand
        X = [rand_seq(rng, K) for _ in range(6)]
        if variant:
            X = [revcomp(x) for x in X]
        once = lambda x: around(rng, x, L)
        head += [tandem_read(rng, X[0], 2, L), tandem_read(rng, X[1], 3, L), once(X[2])]              # representatives
        tail += [once(X[0]), once(X[0]), revcomp(once(X[0])), once(X[1]), tandem_read(rng, X[1], 2, L)]
        tail += [tandem_read(rng, X[2], 2, L), revcomp(tandem_read(rng, X[2], 3, L)), once(X[2])]      # later members
        tail += [tandem_read(rng, X[3], 2, L)]                                                          # the second occurrence is the only other member
        tail += [tandem_read(rng, X[4], 3, L)]
        both = rand_seq(rng, 20) + X[5] + rand_seq(rng, 15) + revcomp(X[5]) + rand_seq(rng, 25)         # both strands in one read
        head += [both]
        tail += [once(X[5]), revcomp(both)]
    bg = background(rng, 300, L)
    seqs = head + bg[:150] + tail + bg[150:]
    check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, ignore_multi=0, caps=(64, 5))
    check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, ignore_multi=1, forced=())


# ---- neighbours in slot order
def test_sequence_boundaries_in_slot_order(ctx, oracle_bin, tmp_path, monkeypatch):
    """one run holds the last k-mer position of read i and the first of read i + 1 (two slots apart: slot 0 of read i + 1 lies between);
    read i + 1 identical to read i (with the 20-mer at both ends: --ignore-multi-kmer 0), and the reverse complement of read i (every
    k-mer shared, positions mirrored, in both halves of the read)"""
    rng = np.random.default_rng(5)
    L = 64
    bg = background(rng, 240, L)
    seqs = []
    for j in range(6):
        X = rand_seq(rng, K)
        if j % 2:
            X = revcomp(X)
        a, b = around(rng, X, L, pos=L - K), around(rng, X, L, pos=0)
        seqs += bg[40 * j:40 * j + 37] + [a, b, around(rng, X, L)]
    ends = rand_seq(rng, K)
    twice = ends + rand_seq(rng, L - 2 * K) + ends
    r = rand_seq(rng, L)
    seqs += [twice, twice, r, revcomp(r), revcomp(r), r, revcomp(twice), twice]
    check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, ignore_multi=0, caps=(64, 3))
    check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, ignore_multi=1, caps=(2,))


def test_whole_sequence_hash_slot_next_to_kmer_slots(ctx, oracle_bin, tmp_path, monkeypatch):
    """reads whose whole-sequence hash tuple stays in slot 0 (tests/golden/extract_uniform/small_hash_L36_k20.txt) next to copies of
    themselves: the run of the hash holds slot 0 of consecutive sequences - exactly one sequence's slots apart -, and slot 0 lies right in
    front of the k-mer slots of its own read"""
    small = open(os.path.join(GOLDEN, "small_hash_L36_k20.txt")).read().split()
    rng = np.random.default_rng(36)
    bg = background(rng, 600, 36)
    seqs = [small[0], small[0]] + bg[:200] + [small[1], small[1], small[1], revcomp(small[1])] + bg[200:400] + [small[2]] + bg[400:] + [small[2], small[3], small[3]]
    check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, caps=(64, 2))
    check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, ignore_multi=0, forced=())
