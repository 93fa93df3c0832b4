"""Device time of cdm_alns_dedup (its kernel_ms: the count pass and its scan, the emit pass, the radix sort of the group keys, the head
flags and their scan, the maximum per run, the keep flags, and over the whole set the placing scan, the offsets and the compaction)
beside cdm_pileup_map's on the same set - the same emit-and-sort skeleton, the only fair neighbour - written to
profiles/contig_dedup.txt:

    python scripts/profile_contig_dedup.py [out.txt] [records:rate ...]        (default: 1000000:0.3 4000000:0.6)

One execution writes the whole file: the header, then the three lines of every (records, rate) pair.  Each set is synthetic: one contig of 3 000 000 letters under `records` reads of 100 letters on both strands, drawn from 64 read sequences;
a share `rate` of the records repeats the strand, start and length of an earlier record (a PCR copy), the others start anywhere (6 M
places on the two strands: some fall on a place already taken, and the removed records the lines print count those too).  Each figure
is the median and the range of 20 calls after 3 warm-up calls.  No speed is claimed: the call is new."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from carpedeam_amd import capi  # noqa: E402

LINES = []


def say(text):
    print(text)
    LINES.append(text)


def synthetic(n, rate, seed=17):
    rng = np.random.default_rng(seed)
    length, rl, targets = 3_000_000, 100, 64
    seqs = ["".join(rng.choice(list("ACGT"), size=length))] + ["".join(rng.choice(list("ACGT"), size=rl)) for _ in range(targets)]
    start = rng.integers(0, length - rl, size=n)
    rev = rng.integers(0, 2, size=n).astype(bool)
    copy = np.flatnonzero(rng.random(n) < rate)
    copy = copy[copy > 0]
    source = (rng.random(len(copy)) * copy).astype(np.int64)          # an earlier record (one that is a copy itself keeps its own draw)
    start[copy], rev[copy] = start[source], rev[source]
    rec = np.zeros(n + 1, capi.ALN_DTYPE)
    rec[0] = (0, 0, 0, 0, length - 1, 0, length - 1, 1.0)
    r = rec[1:]
    r["target"] = 1 + rng.integers(0, targets, size=n)
    r["ident"] = rng.integers(80, 101, size=n)
    r["q_start"] = np.where(rev, start + rl - 1, start)
    r["q_end"] = np.where(rev, start, start + rl - 1)
    r["db_start"], r["db_end"], r["seq_id"] = 0, rl - 1, 1.0
    off = np.full(len(seqs) + 1, n + 1, np.uint64)
    off[0] = 0
    return seqs, off, rec


def timed(call, ms_of):
    ms = []
    for i in range(23):
        out = call()
        if i >= 3:
            ms.append(ms_of())
    return out, float(np.median(ms)), min(ms), max(ms)


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "contig_dedup.txt")
    pairs = [(int(a.split(":")[0]), float(a.split(":")[1])) for a in (sys.argv[2:] or ["1000000:0.3", "4000000:0.6"])]
    ctx = capi.Ctx(0)
    say("contig_dedup (csrc/pileup_dedup.hip, cdm_alns_dedup): the kernels' device time on one MI355X")
    say("=" * 98)
    say("")
    say("One execution of scripts/profile_contig_dedup.py with %s.  The figures are the calls' own kernel_ms (HIP events" % " ".join("%d:%g" % p for p in pairs))
    say("around the stretches of kernels; the radix sort synchronises the stream inside its stretch, so its host gaps are in the figure; the")
    say("uploads, the memsets and the copies back are outside).  Per line 20 calls after 3 warm-up calls: median (min, max).  No speed is")
    say("claimed and no threshold is set: the call is new, there is no figure of the parent commit and none of the reference.")
    say("cdm_pileup_map on the same set stands beside it as the neighbour with the same emit-and-sort skeleton; it also reads the letters of")
    say("every record.")
    for n, rate in pairs:
        seqs, off, rec = synthetic(n, rate)
        db = ctx.upload_seqs(seqs, ext=[1] + [0] * (len(seqs) - 1))
        alns = ctx.upload_alns(db, off, rec)
        say("")
        say("one contig of 3 000 000 letters, %d records of 100 letters, a share of %g repeats an earlier record's strand and start" % (n, rate))
        (_, stats), med, lo, hi = timed(lambda: ctx.alns_dedup(db, alns, [0], 0.0, True), lambda: ctx.dedup_kernel_ms)
        say("  %-32s median %.3f ms (min %.3f, max %.3f)  counted %d kept %d removed %d largest %d" % ("cdm_alns_dedup", med, lo, hi, *[int(x) for x in stats[0]]))
        mstats, med, lo, hi = timed(lambda: ctx.pileup_map(db, alns, [0], 0.0, True), lambda: ctx.map_kernel_ms)
        say("  %-32s median %.3f ms (min %.3f, max %.3f)  reads %d" % ("cdm_pileup_map, statistics alone", med, lo, hi, int(mstats[0][0])))
        out, med, lo, hi = timed(lambda: ctx.pileup_map(db, alns, [0], 0.0, True, records=True), lambda: ctx.map_kernel_ms)
        say("  %-32s median %.3f ms (min %.3f, max %.3f)  records %d" % ("cdm_pileup_map with records", med, lo, hi, len(out[1])))
    say("")
    say("Not measured: the share of each kernel inside kernel_ms (no profiler run was made), batches other than the default (the bound of")
    say("2^26 records a batch is cdm_pileup_map's, reasoned from the bytes a record takes, not measured) and the host side of")
    say("`carpedeam contig_dedup`.")
    with open(path, "w") as f:
        f.write("\n".join(LINES) + "\n")
