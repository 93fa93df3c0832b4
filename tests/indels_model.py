"""cdm_pileup_indels (include/carpedeam_hip.h) in plain Python / numpy, integers only, written twice: indels_brute() goes position by
position and walks every record at each, the yardstick; indels_sorted() is the form of the kernels (difference marks and a prefix sum
for cross, one key per event, a stable sort, runs of equal keys).  Then the check of the caller's records (check_records), the three
texts `carpedeam contig_indels` writes and apply_consensus(), the rule its FASTA follows.  The reference project has nothing like it:
this file is the specification, tests/test_indels_model.py holds its two halves against each other and against planted answers."""
import numpy as np

import map_model as mm
from depth_model import counted
from gapped_model import GAP_DTYPE, OP_D, OP_I, OP_M, REVERSE  # noqa: F401  (GAP_DTYPE: for the users of this module)

NAMES = ("reads", "columns", "rescued", "insertions", "deletions", "inserted_letters", "deleted_letters", "places", "supported", "major")
FIELDS = ("query", "pos", "info", "count", "cross", "others", "n_letters", "reserved")
INDEL_DTYPE = np.dtype([(n, "<u4") for n in FIELDS] + [("letters", "<u8")])
INS, DEL = 1, 2
CALLED, SUPPORTED, MAJOR = 1, 2, 4
MAX_GAP = 62


class Params:
    """cdm_indel_params with the command's values"""

    def __init__(self, min_depth=3, min_count=2, min_percent=20, min_seq_id=0.0, skip=False):
        self.min_depth, self.min_count, self.min_percent, self.min_seq_id, self.skip = min_depth, min_count, min_percent, min_seq_id, skip


# ------------------------------------------------------------------------------------------------ the caller's records
def check_records(seqs, queries, recs, ops):
    """the host's one pass over the records -> None, or (index of the first record that fails, what the message says of it)"""
    for i, r in enumerate(recs):
        k, t = int(r["query"]), int(r["target"])
        if k >= len(queries):
            return i, "its query is not an index into the listed queries"
        if t >= len(seqs):
            return i, "its target is not a sequence of the DB"
        if int(r["tlen"]) != len(seqs[t]):
            return i, "tlen is not the length of its target"
        if i and (int(recs[i - 1]["query"]), int(recs[i - 1]["pos"])) > (k, int(r["pos"])):
            return i, "the records do not ascend by (query, pos)"
        at, n = int(r["ops"]), int(r["n_ops"])
        if n < 1 or at + n > len(ops):
            return i, "its operations are not words of the pool"
        span = columns = 0
        for j in range(n):
            w = int(ops[at + j])
            g, op = w >> 2, w & 3
            if op > OP_D or g < 1:
                return i, "an operation that is not M, I or D of at least one letter"
            if j in (0, n - 1) and op != OP_M:
                return i, "its first or last operation is not M"
            if j and int(ops[at + j - 1]) & 3 == op:
                return i, "two neighbouring operations of one code"
            if op != OP_M and g > MAX_GAP:
                return i, "an insertion or deletion of more than 62 letters"
            span += g if op != OP_I else 0
            columns += g if op != OP_D else 0
        if span != int(r["span"]) or columns != int(r["columns"]):
            return i, "its operations do not sum to span and columns"
        if int(r["pos"]) + span > len(seqs[int(queries[k])]):
            return i, "pos + span lies beyond its query"
        if int(r["tstart"]) + columns > int(r["tlen"]):
            return i, "tstart + columns lies beyond its target"
    return None


def events_of(r, ops):
    """[(p, kind, g, read offset)] of one gapped record, in the order of its operations"""
    p, off, out = int(r["pos"]), int(r["tstart"]), []
    for w in ops[int(r["ops"]):int(r["ops"]) + int(r["n_ops"])]:
        g, op = int(w) >> 2, int(w) & 3
        if op == OP_M:
            p, off = p + g, off + g
        elif op == OP_I:
            out.append((p, INS, g, off))
            off += g
        else:
            out.append((p, DEL, g, off))
            p += g
    return out


def read_letter(codes, r, at):
    """the code 0..3 of the read letter at offset `at` of the read in the query's orientation, 4 where its N bit is set"""
    if int(r["flags"]) & REVERSE:
        c = int(codes[int(r["tlen"]) - 1 - at])
        return 4 if c == 4 else 3 - c
    return int(codes[at])


def flags_of(count, cross, par):
    f = 0
    if cross >= par.min_depth:
        f = CALLED
        if count >= par.min_count and count * 100 >= par.min_percent * cross:
            f |= SUPPORTED
            if 2 * count > cross:
                f |= MAJOR
    return f


def result(stats, tracks, rows):
    """rows: (k, p, kind, g, flags, count, cross, others, [letters]) of the supported places in site order"""
    sites, letters = np.zeros(len(rows), INDEL_DTYPE), []
    for i, (k, p, kind, g, f, count, cross, others, lets) in enumerate(rows):
        sites[i] = (k, p, kind | g << 4 | f << 16, count, cross, others, len(lets), 0, len(letters))
        letters += lets
    return stats, tracks, sites, np.array(letters, np.uint8)


# ------------------------------------------------------------------------------------------------ the yardstick
def indels_brute(seqs, ext, off, rec, queries, grecs, gops, par):
    """-> (stats[nq, 10] uint64, tracks: one uint32 cross vector per listed query, sites: INDEL_DTYPE, letters: uint8)"""
    view = {}

    def codes(t):
        if t not in view:
            view[t] = mm.codes(seqs[t])
        return view[t]

    stats = np.zeros((len(queries), 10), np.uint64)
    tracks, rows = [], []
    for k, q in enumerate(queries):
        L = len(seqs[int(q)])
        plain = counted(seqs, ext, off, rec, int(q), par.min_seq_id, par.skip)
        mine = [r for r in grecs if int(r["query"]) == k]
        cross = np.zeros(L, np.uint32)
        for b in range(1, L):
            cross[b] = sum(1 for qs, qe in plain if qs < b <= qe) + sum(1 for r in mine if int(r["pos"]) < b <= int(r["pos"]) + int(r["span"]) - 1)
        tracks.append(cross)
        st = [len(plain), sum(qe - qs + 1 for qs, qe in plain), len(mine), 0, 0, 0, 0, 0, 0, 0]
        for p in range(L):
            for kind in (INS, DEL):
                found = []          # (g, record, read offset) of every event of this place, walking every record
                for r in mine:
                    found += [(g, r, at) for ep, ek, g, at in events_of(r, gops) if ep == p and ek == kind]
                if not found:
                    continue
                lengths = sorted(set(g for g, _, _ in found))
                counts = [sum(1 for g, _, _ in found if g == length) for length in lengths]
                best = counts.index(max(counts))            # the first of the largest: the smallest g
                g, count = lengths[best], counts[best]
                f = flags_of(count, int(cross[p]), par)
                st[3 if kind == INS else 4] += len(found)
                st[5 if kind == INS else 6] += sum(x for x, _, _ in found)
                st[7] += 1
                st[8] += bool(f & SUPPORTED)
                st[9] += bool(f & MAJOR)
                if not f & SUPPORTED:
                    continue
                lets = []
                if kind == INS:
                    for j in range(g):
                        seen = [read_letter(codes(int(r["target"])), r, at + j) for x, r, at in found if x == g]
                        votes = [seen.count(c) for c in range(4)]
                        lets.append(votes.index(max(votes)) if max(votes) else 4)
                rows.append((k, p, kind, g, f, count, int(cross[p]), len(found) - count, lets))
        stats[k] = st
    return result(stats, tracks, rows)


# ------------------------------------------------------------------------------------------------ the kernels' form
def indels_sorted(seqs, ext, off, rec, queries, grecs, gops, par):
    """the same results from difference marks, event keys query << 31 | p << 7 | (kind - 1) << 6 | g and one stable sort"""
    view = {}

    def codes(t):
        if t not in view:
            view[t] = mm.codes(seqs[t])
        return view[t]

    nq = len(queries)
    stats = np.zeros((nq, 10), np.uint64)
    tracks = []
    for k, q in enumerate(queries):
        L = len(seqs[int(q)])
        plain = counted(seqs, ext, off, rec, int(q), par.min_seq_id, par.skip)
        cells = np.zeros(L + 1, np.int64)
        for qs, qe in plain:
            cells[qs + 1] += 1
            cells[qe + 1] -= 1
        for r in grecs[grecs["query"] == k]:
            cells[int(r["pos"]) + 1] += 1
            cells[int(r["pos"]) + int(r["span"])] -= 1
        assert cells.sum() == 0
        tracks.append(np.cumsum(cells)[:L].astype(np.uint32))
        stats[k][:3] = [len(plain), sum(qe - qs + 1 for qs, qe in plain), int((grecs["query"] == k).sum())]
    keys, ev_rec, ev_off = [], [], []
    for i, r in enumerate(grecs):
        for p, kind, g, at in events_of(r, gops):
            keys.append(int(r["query"]) << 31 | p << 7 | (kind - 1) << 6 | g)
            ev_rec.append(i)
            ev_off.append(at)
            stats[int(r["query"])][3 if kind == INS else 4] += 1
            stats[int(r["query"])][5 if kind == INS else 6] += g
    keys = np.array(keys, np.uint64)
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]
    a_start = np.flatnonzero(np.concatenate(([True], skeys[1:] != skeys[:-1]))) if len(skeys) else np.zeros(0, np.int64)
    a_start = np.concatenate((a_start, [len(skeys)])).astype(np.int64)
    a_keys = skeys[a_start[:-1]]
    p_start = np.flatnonzero(np.concatenate(([True], (a_keys[1:] >> np.uint64(6)) != (a_keys[:-1] >> np.uint64(6))))) if len(a_keys) else np.zeros(0, np.int64)
    p_start = np.concatenate((p_start, [len(a_keys)])).astype(np.int64)
    rows = []
    for pl in range(len(p_start) - 1):
        a0, a1 = int(p_start[pl]), int(p_start[pl + 1])
        counts = a_start[a0 + 1:a1 + 1] - a_start[a0:a1]
        best = a0 + int(np.argmax(counts))          # the first of the largest
        key = int(a_keys[best])
        g, kind, p, k = key & 63, ((key >> 6) & 1) + 1, (key >> 7) & 0xFFFFFF, key >> 31
        count, cross = int(counts[best - a0]), int(tracks[k][p])
        f = flags_of(count, cross, par)
        stats[k][7] += 1
        stats[k][8] += bool(f & SUPPORTED)
        stats[k][9] += bool(f & MAJOR)
        if not f & SUPPORTED:
            continue
        lets = []
        if kind == INS:
            votes = np.zeros((g, 4), np.int64)
            for e in order[int(a_start[best]):int(a_start[best + 1])]:
                r = grecs[ev_rec[e]]
                for j in range(g):
                    c = read_letter(codes(int(r["target"])), r, ev_off[e] + j)
                    if c < 4:
                        votes[j][c] += 1
            lets = [int(np.argmax(v)) if v.max() else 4 for v in votes]
        rows.append((k, p, kind, g, f, count, cross, int(a_start[a1] - a_start[a0]) - count, lets))
    return result(stats, tracks, rows)


# ------------------------------------------------------------------------------------------------ the texts of `carpedeam contig_indels`
HEADER = "name\tkey\tlength\treads\tcolumns\trescued\tinsertions\tdeletions\tinserted_letters\tdeleted_letters\tplaces\tsupported\tmajor\tapplied\tnew_length\n"


def letters_of(site, letters):
    at = int(site["letters"])
    return "".join(mm.LETTERS[int(c)] for c in letters[at:at + int(site["n_letters"])])


def apply_consensus(contig, sites, letters):
    """contig: its letters as in the input; sites: its site records in site order -> (the polished letters, sites applied).  The MAJOR
    sites behind a cursor: a site in front of the cursor lies inside a stretch an earlier deletion removed and is skipped"""
    out, nxt, applied = [], 0, 0
    for s in sites:
        p = int(s["pos"])
        if not (int(s["info"]) >> 16) & MAJOR or p < nxt:
            continue
        out.append(contig[nxt:p])
        applied += 1
        if int(s["info"]) & 15 == INS:
            out.append(letters_of(s, letters))
            nxt = p
        else:
            nxt = p + ((int(s["info"]) >> 4) & 0xFFF)
    out.append(contig[nxt:])
    return "".join(out), applied


def summary_tsv(names, keys, contigs, stats, sites, letters):
    out = [HEADER]
    for i, name in enumerate(names):
        polished, applied = apply_consensus(contigs[i], sites[sites["query"] == i], letters)
        out.append("\t".join([name, str(int(keys[i])), str(len(contigs[i]))] + [str(int(v)) for v in stats[i]] + [str(applied), str(len(polished))]) + "\n")
    return "".join(out)


def sites_tsv(names, contigs, sites, letters):
    """name, pos (1-based), I|D, length, letters (an I: the voted letters; a D: the contig's mapped letters there), count, cross, others, S|SM"""
    out = []
    for s in sites:
        i, p, info = int(s["query"]), int(s["pos"]), int(s["info"])
        kind, g = info & 15, (info >> 4) & 0xFFF
        shown = letters_of(s, letters) if kind == INS else mm.mapped(contigs[i])[p:p + g]
        out.append("%s\t%d\t%s\t%d\t%s\t%d\t%d\t%d\t%s\n" % (names[i], p + 1, "I" if kind == INS else "D", g, shown, int(s["count"]), int(s["cross"]), int(s["others"]),
                                                          "SM" if (info >> 16) & MAJOR else "S"))
    return "".join(out)


def consensus_fasta(names, contigs, sites, letters):
    return "".join(">%s\n%s\n" % (name, apply_consensus(contigs[i], sites[sites["query"] == i], letters)[0]) for i, name in enumerate(names))
