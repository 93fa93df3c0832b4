#!/usr/bin/env python3
"""mergereads on the device against the reference's single-threaded module, on seeded 2 x 150 pairs of ancient-DNA-like fragments
(30-250 bp, read-through into adapter, ~1 % errors):

    python scripts/mergereads_bench.py <pairs> <summary.json> [--threads 16] [--profile-dir DIR]

Prints and writes: the module's wall time and its CDM_TIMING laps (parse / device / write), the merge kernels' device time, the
reference's wall time (oracle/_ref/carpedeam_full, when built), and whether the two outputs are identical.  With --profile-dir, one
more run of the module under `rocprofv3 --kernel-trace --stats` writes its kernel statistics there."""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
REF = os.path.join(ROOT, "oracle", "_ref", "carpedeam_full")
ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCACAGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGTAGATCGGAAGAGCACACGTCTGAACTCCAGTCACAGATCGGAAGAGCGTCGTGTAGGG"
FILES = ["", ".index", ".dbtype", "_h", "_h.index", "_h.dbtype"]


def write_pairs(n, d, read_len=150, seed=1, chunk=500_000):
    """Fixed-width four-line FASTQ records "@p%09d/1" written chunk by chunk with numpy."""
    rng = np.random.default_rng(seed)
    acgt, comp = np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"TGCA", np.uint8)
    ad = np.frombuffer(ADAPTER, np.uint8)[:read_len]
    paths = [os.path.join(d, "R1.fq"), os.path.join(d, "R2.fq")]
    fs = [open(p, "wb") for p in paths]
    cols = np.arange(read_len)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        codes = rng.integers(0, 4, size=(m, 250), dtype=np.uint8)
        fl = rng.integers(30, 251, size=m)
        inside = cols[None, :] < fl[:, None]
        adi = np.clip(cols[None, :] - fl[:, None], 0, read_len - 1)
        r1 = np.where(inside, acgt[codes[:, :read_len]], ad[adi])
        src = np.clip(fl[:, None] - 1 - cols[None, :], 0, 249)
        r2 = np.where(inside, comp[np.take_along_axis(codes, src, 1)], ad[adi])
        for side, r in enumerate((r1, r2)):
            err = rng.random((m, read_len)) < 0.01
            r = np.where(err, acgt[rng.integers(0, 4, size=(m, read_len), dtype=np.uint8)], r)
            q = rng.integers(35, 74, size=(m, read_len), dtype=np.uint8)
            ids = np.char.encode(np.char.mod("@p%09d/" + str(side + 1) + "\n", np.arange(lo, lo + m)))
            name = np.frombuffer(b"".join(ids.tolist()), np.uint8).reshape(m, -1)
            rec = np.concatenate([name, r, np.full((m, 1), 10, np.uint8), np.frombuffer(b"+\n", np.uint8)[None, :].repeat(m, 0), q,
                                  np.full((m, 1), 10, np.uint8)], axis=1)
            fs[side].write(rec.tobytes())
    for f in fs:
        f.close()
    return paths


def digests(out):
    return {s: hashlib.sha256(open(out + s, "rb").read()).hexdigest() for s in FILES}


def timed(args, timeout, env=None):
    t = time.time()
    r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=timeout)
    return time.time() - t, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", type=int)
    ap.add_argument("summary")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--profile-dir")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--step-timeout", type=float, default=None, help="seconds per device / reference run (default: 30 + 3 us per pair, 30 us for the reference)")
    a = ap.parse_args()
    d = tempfile.mkdtemp(dir=a.tmp)
    try:
        t = time.time()
        r1, r2 = write_pairs(a.pairs, d)
        res = {"pairs": a.pairs, "read_len": 150, "input_bytes": os.path.getsize(r1) + os.path.getsize(r2), "generate_s": round(time.time() - t, 2)}
        dev = os.path.join(d, "dev")
        # every child under a time limit of its own: a hang ends the script (subprocess.TimeoutExpired)
        dev_limit = a.step_timeout or 30 + 3e-6 * a.pairs
        ref_limit = a.step_timeout or 30 + 30e-6 * a.pairs
        wall, r = timed([MODULES, "mergereads", r1, r2, dev, "--threads", str(a.threads)], dev_limit, {"CDM_TIMING": "1"})
        if r.returncode:
            sys.exit("device module failed: " + r.stderr[-2000:])
        laps = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"^  (\S[^\n]*?)\s+([0-9.]+) s$", r.stderr, re.M)}
        km = re.search(r"merge kernels ([0-9.]+) ms", r.stderr)
        res.update({"device_module_wall_s": round(wall, 3), "device_module_laps_s": laps, "merge_kernels_ms": float(km.group(1)) if km else None,
                    "entries": int(open(dev + ".index").read().count("\n"))})
        res["merge_kernels_hbm_bound_ms"] = round(a.pairs * 600 / 6e12 * 1e3, 3)      # 2 x 150 letters + 2 x 150 qualities per pair, read once at 6 TB/s
        if os.path.exists(REF):
            ref = os.path.join(d, "ref")
            wall_ref, r = timed([REF, "mergereads", r1, r2, ref, "--threads", "1"], ref_limit)
            if r.returncode:
                sys.exit("reference failed: " + r.stderr[-2000:])
            res.update({"reference_wall_s": round(wall_ref, 3), "speedup": round(wall_ref / wall, 2), "outputs_identical": digests(dev) == digests(ref)})
        if a.profile_dir:
            os.makedirs(a.profile_dir, exist_ok=True)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", a.profile_dir, "-o", "mergereads", "--output-format", "csv", "--",
                                MODULES, "mergereads", r1, r2, os.path.join(d, "prof"), "--threads", str(a.threads)], capture_output=True, text=True,
                               timeout=2 * dev_limit)
            res["rocprofv3_rc"] = r.returncode
        json.dump(res, open(a.summary, "w"), indent=1)
        print(json.dumps(res, indent=1))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
