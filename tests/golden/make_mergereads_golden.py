#!/usr/bin/env python3
"""Generate tests/golden/mergereads/ from the reference's own `mergereads` (oracle/_ref/carpedeam_full, built by
`make -C oracle -f Makefile.ref`).

Inputs are seeded synthetic read pairs (plus the reference's example reads cut into pairs); outputs are the sha256 of every file
the reference writes, and a keyed dump of its entries for diagnosis.

    python tests/golden/make_mergereads_golden.py
"""
import gzip
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.path.join(ROOT, "oracle", "_ref", "carpedeam_full")
OUT = os.path.join(ROOT, "tests", "golden", "mergereads")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example", "test_data.fq.gz")
FILES = ["", ".index", ".dbtype", "_h", "_h.index", "_h.dbtype"]
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def rc(s):
    return "".join(COMP.get(c, "N") for c in reversed(s))


def qual(rng, n, lo=35, hi=73):
    return "".join(chr(rng.randint(lo, hi)) for _ in range(n))


def mutate(rng, s, rate):
    return "".join(rng.choice("ACGT") if rng.random() < rate else c for c in s)


def fq(recs):
    return "".join("@%s\n%s\n+\n%s\n" % r for r in recs).encode()


def adna(rng, n, read_len, adapter="AGATCGGAAGAGCACACGTCTGAACTCCAGTCACAGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"):
    """Fragments of 30-250 bp; reads of read_len from both ends, running into adapter where the fragment is shorter; ~1 % errors."""
    r1s, r2s = [], []
    for k in range(n):
        frag = "".join(rng.choice("ACGT") for _ in range(rng.randint(30, 250)))
        a = (frag + adapter + "A" * read_len)[:read_len]
        b = (rc(frag) + adapter + "A" * read_len)[:read_len]
        r1s.append(("p%d/1 frag=%d" % (k, len(frag)), mutate(rng, a, 0.01), qual(rng, read_len)))
        r2s.append(("p%d/2" % k, mutate(rng, b, 0.01), qual(rng, read_len)))
    return r1s, r2s


def letters(rng):
    """Pairs built for the corner cases of the contract."""
    r1s, r2s = [], []

    def add(name, s1, q1, s2, q2):
        r1s.append((name + "/1", s1, q1)); r2s.append((name + "/2", s2, q2))

    for k in range(120):
        L = rng.randint(20, 160)
        frag = "".join(rng.choice("ACGT") for _ in range(L + rng.randint(0, 80)))
        l1, l2 = rng.randint(5, L), rng.randint(5, L)               # unequal lengths, some < 15
        s1, s2 = frag[:l1], rc(frag)[:l2]
        kind = k % 6
        if kind == 1:      # N-rich
            s1 = "".join("N" if rng.random() < 0.2 else c for c in s1); s2 = "".join("N" if rng.random() < 0.2 else c for c in s2)
        elif kind == 2:    # lower case (a mismatch against upper case), lower-case n (not an N)
            s1 = "".join(c.lower() if rng.random() < 0.1 else c for c in s1); s2 = "".join("n" if rng.random() < 0.05 else c for c in s2)
        elif kind == 3:    # IUPAC codes, U, and bytes that complement to '.'
            s1 = "".join(rng.choice("RYKMSWBDHVU.-*xX") if rng.random() < 0.08 else c for c in s1)
            s2 = "".join(rng.choice("RYKMSWBDHVUryk.-*#") if rng.random() < 0.08 else c for c in s2)
        elif kind == 4:    # many mismatches: densities near 0.1
            s1 = mutate(rng, s1, 0.12); s2 = mutate(rng, s2, 0.12)
        add("c%d" % k, s1, qual(rng, len(s1)), s2, qual(rng, len(s2)))
    # equal-density ties: 2 mismatches in 20 vs 3 in 30 (the same float), decided by quality; and equal (density, quality)
    for k in range(12):
        unit = "".join(rng.choice("ACGT") for _ in range(10))
        s1 = unit * 6
        s2 = rc(mutate(rng, unit * 6, 0.05))
        add("tie%d" % k, s1, qual(rng, len(s1), 40, 42), s2, qual(rng, len(s2), 40, 42))
    # overlaps > 65 (density over 1 possible), equal qualities at mismatches, with and without N
    for k in range(12):
        frag = "".join(rng.choice("ACGT") for _ in range(200))
        s1, s2 = frag[:150], rc(frag[40:])
        s1 = mutate(rng, s1, 0.03)
        if k % 2:
            s2 = "".join("N" if rng.random() < 0.05 else c for c in s2)
        add("eq%d" % k, s1, "I" * len(s1), s2, "I" * len(s2))
    for k in range(6):      # random, unrelated: high densities everywhere
        s1 = "".join(rng.choice("ACGT") for _ in range(150)); s2 = "".join(rng.choice("ACGT") for _ in range(150))
        add("rnd%d" % k, s1, qual(rng, 150), s2, qual(rng, 150))
    return r1s, r2s


def example_pairs(n=None, read_len=60):
    """The reference's example reads cut into pairs: R1 = the first read_len bases, R2 = the reverse complement of the last."""
    recs = []
    lines = gzip.open(EXAMPLE, "rt").read().split("\n")
    for k in range(0, len(lines) - 3, 4):
        recs.append((lines[k][1:].split()[0], lines[k + 1], lines[k + 3]))
    recs = [r for r in recs if len(r[1]) >= 30][:n]
    r1s = [(name + "/1", s[:read_len], q[:read_len]) for name, s, q in recs]
    r2s = [(name + "/2", rc(s[-read_len:]), q[-read_len:][::-1]) for name, s, q in recs]
    return r1s, r2s


def run_case(name, inputs, d):
    """inputs: [(file name, bytes)] in argument order; returns {file suffix: sha256} of the reference's output."""
    paths = []
    for fn, data in inputs:
        p = os.path.join(OUT, name + "." + fn)
        open(p, "wb").write(gzip.compress(data, mtime=0) if fn.endswith(".gz") else data)
        paths.append(p)
    out = os.path.join(d, name)
    r = subprocess.run([REF, "mergereads"] + paths + [out, "--threads", "1"], capture_output=True, text=True)
    if r.returncode:
        sys.exit("%s: %s" % (name, r.stderr[-2000:]))
    res = {s: hashlib.sha256(open(out + s, "rb").read()).hexdigest() for s in FILES}
    # keyed dump: key \t header \t sequence
    from carpedeam_amd import mmdb
    seqs, hdrs = mmdb.read_db(out), mmdb.read_db(out + "_h")
    dump = "".join("%d\t%s\t%s\n" % (k, hdrs[k][0].rstrip(b"\n\0").decode("latin-1"), seqs[k][0].rstrip(b"\n\0").decode("latin-1")) for k in sorted(seqs))
    open(os.path.join(OUT, name + ".keyed.gz"), "wb").write(gzip.compress(dump.encode("latin-1"), mtime=0))
    return res


def workflow(threads=8):
    """example_ancient_assemble.fasta: the reference's whole program on the example pairs - its paired-end way in, mergereads first
    (guidedNuclAssemble.sh:28-32) - as `ancient_assemble example.R1.fq.gz example.R2.fq.gz out.fa tmp --ancient-damage <dhigh>
    --min-contig-len 30`.  (With the default of 500 the reference writes no contig from these 51-bp reads: every mergereads entry
    carries wasExtended = 1, and nothing is extended.)"""
    import shutil
    from carpedeam_amd import synth
    with tempfile.TemporaryDirectory() as tmp:
        synth.write_dhigh_profiles(os.path.join(tmp, "dhigh"))
        out = os.path.join(tmp, "out.fa")
        r = subprocess.run([REF, "ancient_assemble", os.path.join(OUT, "example.R1.fq.gz"), os.path.join(OUT, "example.R2.fq.gz"), out, os.path.join(tmp, "tmp"),
                            "--ancient-damage", os.path.join(tmp, "dhigh"), "--threads", str(threads), "--min-contig-len", "30"], capture_output=True, text=True)
        if r.returncode:
            sys.exit("reference workflow failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        shutil.copyfile(out, os.path.join(OUT, "example_ancient_assemble.fasta"))
    print("workflow golden: %d contigs" % open(os.path.join(OUT, "example_ancient_assemble.fasta")).read().count(">"))


def main():
    sys.path.insert(0, ROOT)
    os.makedirs(OUT, exist_ok=True)
    rng = random.Random(20261016)
    cases = {}
    a1, a2 = adna(rng, 300, 100)
    b1, b2 = adna(rng, 200, 150)
    c1, c2 = letters(rng)
    long1 = "".join(rng.choice("ACGT") for _ in range(5600))
    l1 = [("long/1", mutate(rng, long1[:5000], 0.01), qual(rng, 5000))]
    l2 = [("long/2", mutate(rng, rc(long1[600:]), 0.01), qual(rng, 5000))]
    e1, e2 = example_pairs()
    # two file pairs; the second of different record counts and with a quality line of the wrong length ending its R2
    m1, m2 = adna(rng, 40, 100)
    m2 = m2[:30] + [(m2[30][0], m2[30][1], m2[30][2][:-3])] + m2[31:]
    with tempfile.TemporaryDirectory() as d:
        cases["adna100"] = run_case("adna100", [("R1.fq.gz", fq(a1)), ("R2.fq.gz", fq(a2))], d)
        cases["adna150"] = run_case("adna150", [("R1.fq.gz", fq(b1)), ("R2.fq.gz", fq(b2))], d)
        cases["letters"] = run_case("letters", [("R1.fq.gz", fq(c1)), ("R2.fq.gz", fq(c2))], d)
        cases["long"] = run_case("long", [("R1.fq.gz", fq(l1)), ("R2.fq.gz", fq(l2))], d)
        cases["example"] = run_case("example", [("R1.fq.gz", fq(e1)), ("R2.fq.gz", fq(e2))], d)
        cases["two"] = run_case("two", [("A_R1.fq.gz", fq(a1[:50])), ("A_R2.fq.gz", fq(a2[:45])), ("B_R1.fq.gz", fq(m1)), ("B_R2.fq.gz", fq(m2))], d)
    json.dump(cases, open(os.path.join(OUT, "digests.json"), "w"), indent=1, sort_keys=True)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
    workflow()
