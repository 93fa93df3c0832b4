"""kmermatcher's extraction kernel for plain uniform DBs in the slot layout (kmer_extract.h k_extract_uniform: one kernel instead of
k_seq_hash + k_extract_pair): the hits equal the oracle's at every shape where the kernel can go wrong, under the default (the new kernel
wherever it is chosen), under CDM_EXTRACT=pair (the two old kernels) and under CDM_SLOT_HIST=check (the head histogram the extractor counts
against a count of the keys it wrote)."""
import os

import numpy as np
import pytest

from carpedeam_amd import capi, mmdb
from gpuutil import diff_keys, run_oracle
from stageflags import K_FLAGS

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extract_uniform")
LETTERS = np.frombuffer(b"ACGT", np.uint8)
PALINDROME = "ACGTACGTACGTACGTACGT"         # its own reverse complement: an empty slot at k = 20
UNITS = ("A", "AC", "ACGTTGCA", "ACGTACGTAC")


@pytest.fixture(scope="module")
def ctx():
    return capi.Ctx(0)


def reads(n, L, seed):
    """n reads of L letters off both strands of a random genome at ~20x"""
    rng = np.random.default_rng(seed)
    G = max(2 * L, n * L // 20)
    genome = rng.integers(0, 4, G + L)
    out = []
    for _ in range(n):
        st = int(rng.integers(0, G))
        c = genome[st:st + L]
        if rng.random() < 0.5:
            c = (3 - c)[::-1]
        out.append(LETTERS[c].tobytes().decode())
    return out


def tandem(L):
    return [(u * (L // len(u) + 1))[:L] for u in UNITS]


def with_palindrome(read, at):
    return (read[:at] + PALINDROME + read[at + len(PALINDROME):])[:len(read)]


def check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, k=20, envs=()):
    t = lambda s: str(tmp_path / s)
    mmdb.write_seqdb(t("in"), seqs)
    flags = " ".join(K_FLAGS).replace("-k 20", "-k %d" % k).split()
    run_oracle(oracle_bin, "kmermatcher", t("in"), t("pref"), *flags, "--threads", "2")
    want = {key: (v[0], 0) for key, v in mmdb.read_db(t("pref")).items()}
    keyed = mmdb.read_db(t("in"))
    par = capi.KmerParams(k, 200, 0.2, 67, 1, 0, 1, 0.0)
    for env in ({}, {"CDM_EXTRACT": "pair"}, {"CDM_SLOT_HIST": "check"}) + tuple(envs):
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        db = ctx.upload_keyed_seqdb(keyed)
        _, keys, _ = db.meta()
        off, rec = ctx.kmermatch(db, par).download()
        got = {key: (v, 0) for key, v in capi.hits_to_text(off, rec, keys).items()}
        for name in env:
            monkeypatch.delenv(name)
        assert not diff_keys(got, want), env


# (L, k, n): one k-mer and two slots per read; two k-mers; short and standard reads; 96 positions - the last length a half-wave takes -
# and 97, which k_extract_fast takes (the old kernels); odd numbers of reads throughout: the last half-wave has no read
@pytest.mark.parametrize("L,k,n", [(20, 20, 701), (21, 20, 701), (36, 20, 1501), (100, 20, 2001), (115, 20, 901), (116, 20, 901),
                                   (14, 14, 701), (15, 14, 701), (36, 14, 1501), (100, 14, 1201), (109, 14, 601)])
def test_lengths_and_k(ctx, oracle_bin, tmp_path, monkeypatch, L, k, n):
    seqs = reads(n, L, seed=1000 * L + k)
    seqs += seqs[:n // 20]          # verbatim copies
    if len(seqs) % 2 == 0:
        seqs.pop()
    check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, k)


def test_one_read(ctx, oracle_bin, tmp_path, monkeypatch):
    check(ctx, oracle_bin, tmp_path, monkeypatch, reads(1, 100, seed=3))
    check(ctx, oracle_bin, tmp_path, monkeypatch, reads(2, 36, seed=4))


@pytest.mark.parametrize("L,k", [(100, 20), (36, 20), (100, 14)])
def test_tandem_repeats_and_palindromes(ctx, oracle_bin, tmp_path, monkeypatch, L, k):
    """repeated canonical k-mers (the tag set finds them, k_extract rewrites the read) and k-mers that are their own reverse complement
    (an empty slot), between ordinary reads, at the start, in the middle and at the end of the list"""
    seqs = reads(900, L, seed=L + k)
    rep = tandem(L)
    pal = [with_palindrome(s, at) for s, at in zip(reads(6, L, seed=77), (0, 1, (L - 20) // 2, L - 21, L - 20, 7))] + [(PALINDROME * 6)[:L]]
    seqs = rep + seqs[:300] + pal + rep + seqs[300:] + pal[:3] + rep[:3]
    assert len(seqs) % 2 == 1
    check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, k)


def test_one_n_takes_the_old_kernels(ctx, oracle_bin, tmp_path, monkeypatch):
    """one length, one N: not a plain uniform DB"""
    seqs = reads(1201, 100, seed=9)
    seqs[600] = seqs[600][:40] + "N" + seqs[600][41:]
    check(ctx, oracle_bin, tmp_path, monkeypatch, seqs)


@pytest.mark.parametrize("n,blocks", [(3001, "1"), (2049, "3"), (4097, "2")])
def test_wave_takes_several_batches(ctx, oracle_bin, tmp_path, monkeypatch, n, blocks):
    """a grid of a few blocks (CDM_EXTRACT_BLOCKS): every wave walks several batches of 32 pairs, the read-ahead goes from the end of a
    batch to the wave's next one and, behind the last, past the end of the list; the last batch is not full"""
    seqs = reads(n - 8, 100, seed=n) + tandem(100) * 2
    check(ctx, oracle_bin, tmp_path, monkeypatch, seqs, envs=({"CDM_EXTRACT_BLOCKS": blocks}, {"CDM_EXTRACT_BLOCKS": blocks, "CDM_SLOT_HIST": "check"}))


def test_hash_tuple_that_fits_2k_bits(ctx, oracle_bin, tmp_path, monkeypatch):
    """One read in 2^23 at k = 20 has a whole-sequence hash key below 2^40: its tuple stays in slot 0, in region 1, and its region-2
    slot is empty.  tests/golden/extract_uniform/small_hash_L36_k20.txt holds six such reads of 36 letters (k = 20, seed 67; found by
    scripts/find_small_hash_reads.py in well under a minute of CPU search), here between ordinary reads and next to copies of
    themselves (the copies share the hash: a run of whole-sequence tuples inside region 1)."""
    small = open(os.path.join(GOLDEN, "small_hash_L36_k20.txt")).read().split()
    assert len(small) == 6 and all(len(s) == 36 for s in small)
    seqs = reads(1195, 36, seed=36)
    seqs = small[:2] + seqs[:500] + small[2:5] + small[:1] + seqs[500:] + small[5:] + small[3:4]
    assert len(seqs) % 2 == 1
    check(ctx, oracle_bin, tmp_path, monkeypatch, seqs)
