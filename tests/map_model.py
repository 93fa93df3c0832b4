"""cdm_pileup_map (include/carpedeam_hip.h) in plain numpy / Python, written from the header text: one record per counted record of a
listed query with its mismatch words, coordinate order, one primary record per read, the four statistics; sam_text() is the file
`carpedeam contig_map` writes for such records, and sam_check() verifies a SAM text on its own, from the contigs alone.
tests/test_map_model.py holds all three against hand-computed answers; the device and the command are held against them."""
import re

import numpy as np

import seqdb_model
from pileup_model import orient

NAMES = ("reads", "columns", "mismatches", "primary")
FIELDS = ("query", "target", "pos", "columns", "tstart", "tlen", "nm", "flags")
MAP_DTYPE = np.dtype([(n, "<u4") for n in FIELDS] + [("mm", "<u8")])
REVERSE, SECONDARY = 1, 2
LETTERS = "ACGTN"
COMPLEMENT = str.maketrans("ACGTN", "TGCAN")


def mapped(seq):
    """the letters the DB's codes and N bits stand for (NucleotideMatrix's view, tests/seqdb_model.py), as a str"""
    if isinstance(seq, str):
        seq = seq.encode()
    return seqdb_model.mapped(seq).decode()


def codes(seq):
    """A, C, G, T = 0..3 and 4 where the N bit is set"""
    return np.array([LETTERS.index(c) for c in mapped(seq)], np.int64)


def map_records(seqs, ext, off, rec, queries, min_seq_id=0.0, skip=False):
    """-> (stats[nq, 4] uint64, recs: MAP_DTYPE, mism: uint32) of the listed queries"""
    thr = np.float32(min_seq_id)
    view = {}

    def code_of(i):
        if i not in view:
            view[i] = codes(seqs[i])
        return view[i]

    rows = []           # (k, pos, r, fields..., words)
    for k, q in enumerate(queries):
        q = int(q)
        for r in range(int(off[q]), int(off[q + 1])):
            a = rec[r]
            t = int(a["target"])
            if t == q or not (np.float32(a["seq_id"]) >= thr) or (skip and ext[t]):
                continue
            tlen = len(seqs[t])
            qs, qe, ds, _, rev = orient(a, tlen)
            n = qe - qs + 1
            c = np.arange(n)
            ref = code_of(q)[qs + c]
            p = tlen - 1 - (ds + c) if rev else ds + c
            read = code_of(t)[p]
            if rev:
                read = np.where(read == 4, 4, 3 - read)
            bad = (ref == 4) | (read == 4) | (ref != read)
            words = [int(i) | int(ref[i]) << 24 | int(read[i]) << 28 for i in np.flatnonzero(bad)]
            rows.append(dict(k=k, r=r, target=t, pos=qs, columns=n, tstart=ds, tlen=tlen, rev=rev, words=words))
    best = {}           # per target: the most columns, among equals the smallest index in the set
    for row in rows:
        key = (row["columns"], -row["r"])
        if row["target"] not in best or key > best[row["target"]]:
            best[row["target"]] = key
    rows.sort(key=lambda row: (row["k"], row["pos"], row["r"]))
    stats = np.zeros((len(queries), 4), np.uint64)
    recs = np.zeros(len(rows), MAP_DTYPE)
    mism = []
    for i, row in enumerate(rows):
        primary = best[row["target"]] == (row["columns"], -row["r"])
        flags = (REVERSE if row["rev"] else 0) | (0 if primary else SECONDARY)
        recs[i] = (row["k"], row["target"], row["pos"], row["columns"], row["tstart"], row["tlen"], len(row["words"]), flags, len(mism))
        mism += row["words"]
        stats[row["k"]] += np.array([1, row["columns"], len(row["words"]), primary], np.uint64)
    return stats, recs, np.array(mism, np.uint32)


# ------------------------------------------------------------------------------------------------ the text of `carpedeam contig_map`
def md_of(words, columns):
    """match-run length, then the contig's letter: begins and ends with a number, a 0 between adjacent mismatches"""
    out, at = [], 0
    for w in words:
        c = int(w) & 0xFFFFFF
        out.append("%d%s" % (c - at, LETTERS[(int(w) >> 24) & 15]))
        at = c + 1
    return "".join(out) + str(columns - at)


def sam_text(contig_names, contig_lengths, read_name, read_seq, recs, mism, read_group=None, primary_only=False):
    """read_name(target) / read_seq(target): the name and the ASCII letters of the read with that index in the joint DB"""
    out = ["@HD\tVN:1.6\tSO:coordinate\n"]
    out += ["@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in zip(contig_names, contig_lengths)]
    if read_group is not None:
        out.append("@RG\tID:%s\n" % read_group)
    out.append("@PG\tID:carpedeam\tPN:carpedeam\n")
    for r in recs:
        flags = int(r["flags"])
        if primary_only and flags & SECONDARY:
            continue
        t, left, n, tlen = int(r["target"]), int(r["tstart"]), int(r["columns"]), int(r["tlen"])
        seq = mapped(read_seq(t))
        assert len(seq) == tlen
        if flags & REVERSE:
            seq = seq.translate(COMPLEMENT)[::-1]
        right = tlen - left - n
        cigar = ("%dS" % left if left else "") + "%dM" % n + ("%dS" % right if right else "")
        words = mism[int(r["mm"]):int(r["mm"]) + int(r["nm"])]
        f = [read_name(t), str((16 if flags & REVERSE else 0) | (256 if flags & SECONDARY else 0)), contig_names[int(r["query"])], str(int(r["pos"]) + 1), "255", cigar, "*", "0", "0",
             seq, "*", "NM:i:%d" % int(r["nm"]), "MD:Z:" + md_of(words, n)]
        if read_group is not None:
            f.append("RG:Z:" + read_group)
        out.append("\t".join(f) + "\n")
    return "".join(out)


CIGAR = re.compile(r"^(?:(\d+)S)?(\d+)M(?:(\d+)S)?$")
MD = re.compile(r"^\d+(?:[ACGTN]\d+)*$")


def sam_check(text, contigs):
    """contigs: {name: ASCII letters}.  Raises ValueError naming the first line that does not hold: the clips and M sum to len(SEQ); SEQ
    and MD rebuild the contig's mapped letters at POS..; a match column holds no N, a mismatch column differs or holds an N; NM is the
    number of letters in MD; the lines are sorted by (@SQ order, POS); every QNAME has exactly one line without 256"""
    order, primaries, last = {}, {}, (-1, -1)
    for no, line in enumerate(text.split("\n")[:-1], 1):
        def fail(what):
            raise ValueError("line %d: %s: %s" % (no, what, line[:200]))
        f = line.split("\t")
        if line.startswith("@"):
            if f[0] == "@SQ":
                name = f[1][3:]
                if name in order:
                    fail("@SQ twice")
                if name not in contigs or int(f[2][3:]) != len(contigs[name]):
                    fail("@SQ names no contig of that length")
                order[name] = len(order)
            continue
        if len(f) < 13:
            fail("fewer than 13 fields")
        qname, flag, rname, pos, cigar, seq = f[0], int(f[1]), f[2], int(f[3]), f[5], f[9]
        tags = dict((t[:5], t[5:]) for t in f[11:])
        m = CIGAR.match(cigar)
        if not m or rname not in order or "NM:i:" not in tags or "MD:Z:" not in tags or not MD.match(tags["MD:Z:"]):
            fail("malformed")
        left, n, right = (int(x) if x else 0 for x in m.groups())
        if left + n + right != len(seq) or n == 0:
            fail("the clips and M do not sum to len(SEQ)")
        ref = mapped(contigs[rname])
        if pos < 1 or pos - 1 + n > len(ref):
            fail("beyond the contig")
        aligned, rebuilt, at = seq[left:left + n], [], 0
        for run, letter in re.findall(r"(\d+)([ACGTN]?)", tags["MD:Z:"]):
            run = int(run)
            if "N" in aligned[at:at + run]:
                fail("an N in a match run")
            rebuilt.append(aligned[at:at + run])
            at += run
            if letter:
                if at >= n or (letter == aligned[at] and letter != "N"):
                    fail("a mismatch column that matches")
                rebuilt.append(letter)
                at += 1
        if at != n or "".join(rebuilt) != ref[pos - 1:pos - 1 + n]:
            fail("SEQ and MD do not rebuild the contig")
        if int(tags["NM:i:"]) != len(re.findall(r"[ACGTN]", tags["MD:Z:"])):
            fail("NM is not the number of letters in MD")
        if (order[rname], pos) < last:
            fail("not sorted by (@SQ order, POS)")
        last = (order[rname], pos)
        primaries[qname] = primaries.get(qname, 0) + (0 if flag & 256 else 1)
    for qname, n in primaries.items():
        if n != 1:
            raise ValueError("%s has %d lines without 256" % (qname, n))
    return len(primaries)
