"""Reads whose whole-sequence hash tuple stays in slot 0 of the slot layout: XXH64(Util::hash(read), seed) without its top bit fits the 2k
bits of a k-mer - one random read in 2^(63 - 2k).  A seeded CPU search (numpy: the Horner sum h = h * 31 + c over MMseqs2's A,C,T,G = 0..3
letters, then XXH64 of the 8-byte sum) that writes the first `count` such reads, one per line:

    python scripts/find_small_hash_reads.py [L] [k] [count] [seed] > tests/golden/extract_uniform/small_hash_L36_k20.txt
"""
import sys
import time

import numpy as np

L, k, count, seed = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 36), (2, 20), (3, 6), (4, 67)))
M = np.uint64
P1, P2, P3, P4, P5 = (M(x) for x in (11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261))


def rotl(x, r):
    return (x << M(r)) | (x >> M(64 - r))


def xxh64_u64(v, seed):
    h = M(seed) + P5 + M(8)
    k1 = rotl(v * P2, 31) * P1
    h = rotl(h ^ k1, 27) * P1 + P4
    h ^= h >> M(33)
    h *= P2
    h ^= h >> M(29)
    h *= P3
    h ^= h >> M(32)
    return h


rng = np.random.default_rng(20260119)
letters = np.frombuffer(b"ACTG", np.uint8)          # MMseqs2's numeric order
found, tried, t0 = [], 0, time.time()
with np.errstate(over="ignore"):
    while len(found) < count:
        c = rng.integers(0, 4, (1 << 20, L), dtype=np.uint8)
        h = np.zeros(1 << 20, M)
        for i in range(L):
            h = h * M(31) + c[:, i].astype(M)
        key = xxh64_u64(h, seed) & M((1 << 63) - 1)
        for r in np.nonzero(key < M(1 << (2 * k)))[0]:
            found.append(letters[c[r]].tobytes().decode())
        tried += 1 << 20
for s in found[:count]:
    print(s)
sys.stderr.write("%d reads tried, %.1f s\n" % (tried, time.time() - t0))
