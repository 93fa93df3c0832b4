#!/usr/bin/env python3
"""Seeded CPU search for pile-ups on which mostLikeliBaseRead's arg-max hangs on the last bits of its long double sums.

    python scripts/find_call_ties.py            # -> tests/golden/functions/call_ties.tsv.gz, prints the yield

Sparse pile-ups (1..6 non-zero slots of the 44; counts up to 15, 64, 1000 and 65535; reverse counts; all eleven damage classes;
read and extended queries; every query class) go through the long double model of tests/callmodel.py.  Kept are
  (a) exact ties of the top two sums (the first maximum wins),
  (b) near ties: the top two differ by less than 1e-12 relative (the margin below which the kernel leaves plain double) and are not equal,
  (c) vectors whose arg-max differs when the sums are folded in float64.
Most vectors are drawn freely.  The ties they turn up have one shape: every record holds the same base on the same strand (reverse
count mirrors the count, or is zero) and two candidates meet equal table entries, so their sums agree up to the rounding of the
order of summation.  The second draw makes only that shape - one target base, one strand, 1..4 classes.  A share of both draws has
45000..65535 records in a slot, the most the debug hook's 16-bit fields take.  Everything found is written, with the model's answer and the kinds, in the line
format of mostlikeli.tsv.gz plus a third column.
"""
import argparse
import gzip
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import callmodel  # noqa: E402

CAPS = (15, 64, 1000, 65535)


def draw(rs, n, mirrored, heavy):
    cnt, rev = np.zeros((n, 44), np.int64), np.zeros((n, 44), np.int64)
    rows = np.arange(n)
    cap = np.array(CAPS)[rs.randint(0, 4, n)]
    nslots = rs.randint(1, 7, n) if not mirrored else rs.randint(1, 5, n)
    one_base, one_strand = rs.randint(0, 4, n), rs.random_sample(n) < 0.7
    for k in range(6):
        on = k < nslots
        slot = rs.randint(0, 44, n)
        c = (1 + (rs.random_sample(n) ** 2 * cap).astype(np.int64)).clip(1, cap)
        if heavy:
            c = np.where((k == 0), rs.randint(45000, 65536, n), c)
        nr = np.where(rs.random_sample(n) < 0.4, 0, np.where(rs.random_sample(n) < 0.3, c, (rs.random_sample(n) * (c + 1)).astype(np.int64)))
        if mirrored:
            slot = one_base * 11 + slot % 11
            nr = np.where(one_strand, c, 0)
        free = on & (cnt[rows, slot] == 0)
        cnt[rows[free], slot[free]] = c[free]
        rev[rows[free], slot[free]] = nr[free]
    qlen = rs.randint(30, 200, n)
    ends = rs.random_sample(n) < 0.6
    qiter = np.where(ends, np.where(rs.random_sample(n) < 0.5, rs.randint(0, 6, n), qlen - 1 - rs.randint(0, 6, n)), (rs.random_sample(n) * qlen).astype(np.int64))
    head = np.stack([rs.randint(0, 4, n), qiter, qlen, (rs.random_sample(n) < 0.5).astype(np.int64)], 1)
    keep = cnt.sum(1) >= 2
    return head[keep], cnt[keep], rev[keep]


def classify(model, head, cnt, rev):
    ans, s, early = model.call(head[:, 0], head[:, 1], head[:, 2], head[:, 3], cnt, rev)
    ans64, _, _ = model.call(head[:, 0], head[:, 1], head[:, 2], head[:, 3], cnt, rev, dtype=np.float64)
    top = np.sort(s, 1)
    t1, t2 = top[:, 3], top[:, 2]
    a = ~early & (t1 == t2)
    b = ~early & ~a & (t1 - t2 < np.longdouble(1e-12) * (np.abs(t1) + np.abs(t2)))
    c = ~early & (ans64 != ans)
    return ans, s, early, a, b, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--free", type=int, default=400000, help="freely drawn vectors")
    ap.add_argument("--mirrored", type=int, default=100000, help="vectors of one target base on one strand")
    ap.add_argument("--heavy", type=float, default=0.1, help="share with 45000..65535 records in a slot")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "functions", "call_ties.tsv.gz"))
    args = ap.parse_args()
    if not callmodel.usable():
        sys.exit("needs an x87 long double")
    rs = np.random.RandomState(args.seed)
    model = callmodel.Model()
    lines, table = [], []
    for label, total, mirrored in (("free", args.free, False), ("one base, one strand", args.mirrored, True)):
        for heavy in (False, True):
            left = int(total * (args.heavy if heavy else 1 - args.heavy))
            tried = called = 0
            found = {"a": 0, "b": 0, "c": 0}
            pairs = set()
            while left > 0:
                n = min(left, 50000)
                left -= n
                head, cnt, rev = draw(rs, n, mirrored, heavy)
                ans, s, early, a, b, c = classify(model, head, cnt, rev)
                tried += len(head)
                called += int((~early).sum())
                for i in np.nonzero(a | b | c)[0]:
                    kinds = "".join(k for k, m in (("a", a), ("b", b), ("c", c)) if m[i])
                    for k in kinds:
                        found[k] += 1
                    if a[i]:
                        pairs.add(tuple(sorted(np.argsort(-s[i], kind="stable")[:2].tolist())))
                    lines.append("%s\t%d\t%s" % (" ".join(map(str, head[i].tolist() + cnt[i].tolist() + rev[i].tolist())), ans[i], kinds))
            table.append((label + (" heavy" if heavy else ""), tried, called, found["a"], found["b"], found["c"], sorted(pairs)))
    with gzip.GzipFile(args.out, "wb", mtime=0) as f:
        f.write(("\n".join(lines) + "\n").encode())
    print("| draw | vectors | past the 2/5 rule | (a) exact ties | (b) near ties | (c) float64 differs | tied pairs (a) |")
    print("|---|---|---|---|---|---|---|")
    for row in table:
        print("| %s | %d | %d | %d | %d | %d | %s |" % (row[:6] + (" ".join("ACGT"[x] + "ACGT"[y] for x, y in row[6]),)))
    print("%d vectors written to %s (%d bytes)" % (len(lines), os.path.relpath(args.out, ROOT), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
