#!/usr/bin/env python3
"""Contig DBs with prefilter lists for linclust's `align`, and the wall time of the module on them.

    python scripts/align_bench.py --families 30,300,2400 --threads 16 --repeats 3 --out DIR [--ref oracle/_ref/carpedeam_full]

make_db() is the generator (tests/test_gpu_align.py uses it too): families of a random base contig and variants of it (substitutions,
insertions and deletions, a reverse complement, a rotation, a fragment), every ordered pair of a family as a prefilter hit.  The hit's
diagonal is found the way kmermatcher finds it - one shared k-mer - so the DB needs no other program: a line is
"target \\t score \\t diagonal", a negative score marks a reverse-strand hit (a prefilter DB of type 14).

The timing part runs the module on each size with CDM_ALIGN=host, with the reference's binary (if given) and with CDM_ALIGN=device,
alternating, `repeats` times each, and prints the walls, their spread, the device path's CDM_TIMING line and whether the texts agree.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from carpedeam_amd import mmdb  # noqa: E402

ALIGN_FLAGS = ("-a 0 --alignment-mode 2 --alignment-output-mode 0 --wrapped-scoring 1 -e 0.001 --min-seq-id 0.9 --min-aln-len 0 --seq-id-mode 0 --alt-ali 0 -c 0.8 --cov-mode 1 "
               "--max-seq-len 200000 --comp-bias-corr 1 --max-rejected 2147483647 --max-accept 2147483647 --add-self-matches 0 --db-load-mode 0 --pca 1 --pcb 1.5 --score-bias 0 "
               "--realign 0 --realign-score-bias -0.2 --realign-max-seqs 2147483647 --gap-open 5 --gap-extend 2 --zdrop 200 --compressed 0 -v 0").split()
RUN_TIMEOUT = 600         # seconds for one run of a module
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(_RC)[::-1]


def mutate(rng, a, sub, indel):
    """a: uint8 array of letters 0..3; substitutions at rate sub, insertions and deletions at rate indel / 2 each"""
    n = len(a)
    b = np.where(rng.random(n) < sub, rng.integers(0, 4, n, dtype=np.uint8), a)
    out = np.full(2 * n, 255, np.uint8)
    out[0::2] = np.where(rng.random(n) < indel / 2, rng.integers(0, 4, n, dtype=np.uint8), 255)
    out[1::2] = np.where(rng.random(n) >= indel / 2, b, 255)
    return out[out != 255]


def find_diagonal(q, t, wrapped, k=24, tries=12):
    """(reverse, diagonal) of one k-mer the target shares with the query (or its reverse complement), None if none of `tries` does"""
    if len(t) < k or len(q) < k:
        return None
    for reverse, qq in ((False, q), (True, revcomp(q))):
        hay = qq + qq[:k - 1] if wrapped else qq
        for i in range(tries):
            tp = (len(t) - k) * i // max(1, tries - 1)
            qp = hay.find(t[tp:tp + k])
            if qp >= 0:
                d = (qp - tp) % len(qq) if wrapped else qp - tp
                if -32768 <= d < 32768 or (wrapped and d < 65536):
                    return reverse, d
    return None


def make_db(seed, families, lo, hi, variants=3, wrapped=True, rate_scale=1.0):
    """-> (sequences as bytes, prefilter entries [(key, payload)]) of `families` families of contigs of lo..hi letters; rate_scale multiplies
    the mutation rates (short contigs need more to differ at all)"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    seqs, fam = [], []
    for f in range(families):
        base = rng.integers(0, 4, int(rng.integers(lo, hi + 1)), dtype=np.uint8)
        members = [letters[base].tobytes()]
        for _ in range(variants):
            v = letters[mutate(rng, base, rate_scale * [0.002, 0.005, 0.01, 0.02][rng.integers(0, 4)], rate_scale * [0.001, 0.003, 0.006, 0.01][rng.integers(0, 4)])].tobytes()
            kind = int(rng.integers(0, 4))
            if kind == 1:
                v = revcomp(v)
            elif kind == 2 and wrapped and len(v) > 40:
                c = int(rng.integers(1, len(v)))
                v = v[c:] + v[:c]
            elif kind == 3 and len(v) > 60:
                a = int(rng.integers(0, len(v) // 8 + 1))
                v = v[a:a + int(len(v) * rng.uniform(0.85, 1.0))]
            members.append(v)
        for m in members:
            fam.append(f)
            seqs.append(m)
    order = rng.permutation(len(seqs))
    seqs = [seqs[i] for i in order]
    fam = [fam[i] for i in order]
    by_family = {}
    for key, f in enumerate(fam):
        by_family.setdefault(f, []).append(key)
    pref = []
    for key, f in enumerate(fam):
        lines = ["%d\t100\t0\n" % key]
        for other in by_family[f]:
            if other == key:
                continue
            hit = find_diagonal(seqs[key], seqs[other], wrapped)
            if hit is not None:
                lines.append("%d\t%d\t%d\n" % (other, -100 if hit[0] else 100, hit[1] if hit[1] < 32768 else hit[1] - 65536))
        pref.append((key, "".join(lines).encode()))
    return seqs, pref


def write_db(prefix, seqs, pref):
    mmdb.write_seqdb(prefix + "_seq", seqs)
    mmdb.write_db(prefix + "_pref", pref, mmdb.DBTYPE_PREFILTER_REV_RES)


def run_align(binary, prefix, out, threads, env_extra):
    env = dict(os.environ)
    env.pop("CDM_ALIGN", None)
    env.update(env_extra)
    t0 = time.perf_counter()
    r = subprocess.run([binary, "align", prefix + "_seq", prefix + "_seq", prefix + "_pref", out] + ALIGN_FLAGS + ["--threads", str(threads)], capture_output=True, text=True, env=env, timeout=RUN_TIMEOUT)
    wall = time.perf_counter() - t0
    if r.returncode:
        raise RuntimeError("%s align failed (%d): %s" % (binary, r.returncode, r.stderr[-1500:]))
    line = [l.strip() for l in r.stderr.split("\n") if l.strip().startswith("align: path=")]
    return wall, (line[0] if line else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", default="30,300,2400")
    ap.add_argument("--lo", type=int, default=1000)
    ap.add_argument("--hi", type=int, default=5000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", required=True)
    ap.add_argument("--ref", default="")
    ap.add_argument("--paths", default="host,ref,device")
    ap.add_argument("--keep", action="store_true", help="leave the sequence and prefilter DBs of every size in --out")
    a = ap.parse_args()
    exe = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
    os.makedirs(a.out, exist_ok=True)
    report = []
    for families in [int(x) for x in a.families.split(",")]:
        prefix = os.path.join(a.out, "f%d" % families)
        t0 = time.perf_counter()
        seqs, pref = make_db(a.seed, families, a.lo, a.hi)
        write_db(prefix, seqs, pref)
        hits = sum(p.count(b"\n") for _, p in pref)
        print("families %d: %d contigs, %d letters, %d prefilter hits (generated in %.1f s)" % (families, len(seqs), sum(map(len, seqs)), hits, time.perf_counter() - t0), flush=True)
        walls, line = {}, ""
        for rep in range(a.repeats):
            for path in a.paths.split(","):
                if path == "ref" and not a.ref:
                    continue
                binary = a.ref if path == "ref" else exe
                env = {} if path == "ref" else {"CDM_ALIGN": path, "CDM_TIMING": "1"}
                w, l = run_align(binary, prefix, prefix + "_" + path, a.threads, env)
                walls.setdefault(path, []).append(w)
                if path == "device":
                    line = l
                print("  %-6s run %d: %.3f s  %s" % (path, rep + 1, w, l), flush=True)
        texts = {p: mmdb.read_db(prefix + "_" + p) for p in walls}
        entry = {"families": families, "contigs": len(seqs), "letters": sum(map(len, seqs)), "hits": hits, "threads": a.threads, "device_line": line,
                 "walls": {p: {"median": float(np.median(w)), "min": min(w), "max": max(w)} for p, w in walls.items()},
                 "device_equals_host": texts.get("device") == texts.get("host") if "device" in texts and "host" in texts else None,
                 "device_equals_ref": texts.get("device") == texts.get("ref") if "device" in texts and "ref" in texts else None}
        report.append(entry)
        print(json.dumps(entry), flush=True)
        for p in list(walls) + ([] if a.keep else ["seq", "pref"]):
            for suffix in ("", ".index", ".dbtype"):
                if os.path.exists(prefix + "_" + p + suffix):
                    os.remove(prefix + "_" + p + suffix)
    with open(os.path.join(a.out, "align_bench.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
