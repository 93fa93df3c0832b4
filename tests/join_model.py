"""cdm_pileup_junctions (include/carpedeam_hip.h) and the host rules of `carpedeam contig_join` (csrc/host/contig_join.h) in plain Python,
written from the two texts, on top of tests/links_model.py: the pairs of cdm_pileup_links with their letters, the overlap count, the
vote, the decisions A W C X S O J, the paths, and the three files the command writes.  tests/test_join_model.py holds the model against
expectations written out by hand; the device, the host unit and the command are held against it."""
import numpy as np

import links_model as lm

JUNCTION_DTYPE = np.dtype([(n, "<u4") for n in ("a", "b", "info")] + [("gap", "<i4")])
RES_DTYPE = np.dtype([(n, "<u4") for n in ("columns", "matches", "voters", "flags")] + [("fill_off", "<u8")] + [(n, "<u4") for n in ("fill_len", "fill_min", "fill_n", "reserved")])
CONTAINED = 1
DEFAULTS = dict(anchor=16, overhang=1, max_ends=16, min_link_reads=2, overlap_percent=90)
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
# the reverse complement on bytes: case kept, the IUPAC pairs, S W N and every other byte unchanged
_BYTES = dict(zip("ATCGRYKMBVDH", "TAGCYRMKVBHD"))
_BYTES.update({k.lower(): v.lower() for k, v in list(_BYTES.items())})


def device_letters(s):
    """a sequence as the device holds it: A C G T, everything else N"""
    return "".join(c if c in "ACGT" else "N" for c in s.upper())


def rc(s):
    """reverse complement of device letters: N stays N"""
    return "".join(_COMP.get(c, "N") for c in reversed(s))


def rc_bytes(s):
    """reverse complement of a contig's own bytes"""
    return "".join(_BYTES.get(c, c) for c in reversed(s))


def pairs(seqs, ext, off, rec, queries, anchor=16, overhang=1, max_ends=16, min_seq_id=0.0, skip=False, **_):
    """every pair of cdm_pileup_links' rule -> [((a, oA, b, oB), gap, letters)]; letters: the read's letters between the two queries as the
    canonical edge reads them ('' unless gap > 0)"""
    thr = np.float32(min_seq_id)
    ends = {}
    for x, q in enumerate(queries):
        q = int(q)
        q_len = len(seqs[q])
        for r in rec[int(off[q]):int(off[q + 1])]:
            c = lm.counted(seqs, ext, q, r, thr, skip)
            if c is None:
                continue
            qs, qe, ds, de, rev, t_len = c
            u = qs - ds
            L, R = max(0, -u), max(0, u + t_len - q_len)
            if qe - qs + 1 < anchor:
                continue
            left, right = L >= overhang, R >= overhang
            if left != right:
                ends.setdefault(int(r["target"]), []).append((x, right != rev, rev, L if left else R))
    out = []
    for t, e in ends.items():
        if len(e) > max_ends:
            continue
        read = device_letters(seqs[t])
        for x, tail_x, rev_x, h_x in e:
            if not tail_x:
                continue
            for y, tail_y, rev_y, h_y in e:
                if tail_y or x == y:
                    continue
                gap = h_x + h_y - len(read)
                between = read[len(read) - h_x:h_y] if gap > 0 else ""
                if x < y:
                    out.append(((x, int(rev_x), y, int(rev_y)), gap, between))
                else:
                    out.append(((y, int(not rev_y), x, int(not rev_x)), gap, rc(between)))
    return out


def oriented(s, minus):
    return rc(s) if minus else s


def junctions(seqs, ext, off, rec, queries, juncs, **par):
    """-> (res: RES_DTYPE, letters: uint8, counts[letters, 5] uint32)"""
    by_edge = {}
    for key, gap, between in pairs(seqs, ext, off, rec, queries, **par):
        by_edge.setdefault((key, gap), []).append(between)
    res = np.zeros(len(juncs), RES_DTYPE)
    letters, counts = [], []
    for i, j in enumerate(juncs):
        a, b, info, gap = int(j["a"]), int(j["b"]), int(j["info"]), int(j["gap"])
        A, B = device_letters(seqs[int(queries[a])]), device_letters(seqs[int(queries[b])])
        voters = by_edge.get(((a, info & 1, b, info >> 1), gap), [])
        r = res[i]
        r["voters"] = len(voters)
        r["fill_off"] = len(letters)
        if gap < 0:
            k = -gap
            if k > min(len(A), len(B)):
                r["flags"] = CONTAINED
            else:
                oa, ob = oriented(A, info & 1), oriented(B, info & 2)
                r["columns"] = k
                r["matches"] = sum(1 for x, y in zip(oa[len(oa) - k:], ob[:k]) if x == y and x != "N")
        elif gap > 0:
            wins = []
            for o in range(gap):
                c = [sum(1 for v in voters if v[o] == ch) for ch in "ACGTN"]
                best = max(range(4), key=lambda k: (c[k], -k))
                wins.append(c[best])
                letters.append("ACGT"[best] if c[best] else "N")
                counts.append(c)
            r["fill_len"] = gap
            r["fill_min"] = min(wins)
            r["fill_n"] = sum(1 for w in wins if not w)
    return res, np.frombuffer("".join(letters).encode(), np.uint8).copy(), np.array(counts, np.uint32).reshape(-1, 5)


# ------------------------------------------------------------------------------------------------------ the host rules
def link_ends(k):
    """the two contig ends a link touches: (contig, 'R' | 'L')"""
    info = int(k["info"])
    return (int(k["a"]), "L" if info & 1 else "R"), (int(k["b"]), "R" if info & 2 else "L")


def first_decisions(links, lens, min_link_reads=2):
    """steps 1 to 3 -> (decisions: 'A' 'W' 'C' or None per link, junctions: JUNCTION_DTYPE of the links that passed, their link indices)"""
    touched = {}
    for k in links:
        for e in link_ends(k):
            touched[e] = touched.get(e, 0) + 1
    dec = []
    for k in links:
        ea, eb = link_ends(k)
        if touched[ea] > 1 or touched[eb] > 1:
            dec.append("A")
        elif int(k["mode_reads"]) < min_link_reads:
            dec.append("W")
        elif -int(k["gap_mode"]) > min(lens[int(k["a"])], lens[int(k["b"])]):
            dec.append("C")
        else:
            dec.append(None)
    at = [i for i, d in enumerate(dec) if d is None]
    juncs = np.array([(int(links[i]["a"]), int(links[i]["b"]), int(links[i]["info"]), int(links[i]["gap_mode"])) for i in at], JUNCTION_DTYPE) if at else np.empty(0, JUNCTION_DTYPE)
    return dec, juncs, at


def decide(links, lens, dec, at, res, letters, overlap_percent=90):
    """steps 4 to 7 and the paths -> (decisions, paths); a path is a list of members (contig, o, trim, fill letters in front of it), and
    link_path[i] the index of the path of a J link.  res and letters: cdm_pileup_junctions' of the junctions of first_decisions()"""
    dec = list(dec)
    fill = {}
    for r, i in zip(res, at):
        if int(links[i]["gap_mode"]) < 0 and int(r["matches"]) * 100 < overlap_percent * int(r["columns"]):
            dec[i] = "X"
        fill[i] = bytes(letters[int(r["fill_off"]):int(r["fill_off"]) + int(r["fill_len"])]).decode()
    at_end = {}             # (contig, end) -> link

    def remaining():
        at_end.clear()
        for i, k in enumerate(links):
            if dec[i] is None:
                for e in link_ends(k):
                    at_end[e] = i

    remaining()
    for c in range(len(lens)):
        l, r = at_end.get((c, "L")), at_end.get((c, "R"))
        if l is None or r is None:
            continue
        if max(0, -int(links[l]["gap_mode"])) + max(0, -int(links[r]["gap_mode"])) > lens[c]:
            lo, hi = min(l, r), max(l, r)
            dec[lo if int(links[lo]["reads"]) < int(links[hi]["reads"]) else hi] = "S"
            remaining()

    def step(c, o):
        """from contig c in orientation o through its leaving end: (link, next contig, its orientation) or None"""
        i = at_end.get((c, "R" if o == "+" else "L"))
        if i is None:
            return None
        k = links[i]
        info = int(k["info"])
        ea, _ = link_ends(k)
        if ea == (c, "R" if o == "+" else "L") and int(k["a"]) == c:
            return i, int(k["b"]), "-" if info & 2 else "+", True
        return i, int(k["a"]), "+" if info & 1 else "-", False

    seen = set()
    for c in range(len(lens)):          # circles: the smallest index first, +, leaving through its right end
        if c in seen:
            continue
        cur, o, members = c, "+", [c]
        while True:
            s = step(cur, o)
            if s is None:
                break
            _, cur, o, _ = s
            if cur == c:
                dec[at_end[(c, "L")]] = "O"
                remaining()
                break
            if cur in seen:             # an open path that an earlier walk went along already: no circle
                break
            members.append(cur)
        seen.update(members)
    paths, link_path = [], {}
    done = set()
    for c in range(len(lens)):
        if c in done:
            continue
        l, r = at_end.get((c, "L")), at_end.get((c, "R"))
        if (l is None) == (r is None):          # no link, or an inner contig: its path starts at an end contig with a smaller or larger index
            if l is None:
                done.add(c)
            continue
        # an end contig; the other end of its path decides whether it starts
        o = "+" if r is not None else "-"
        members, cur, co = [(c, o, 0, "")], c, o
        used = []
        while True:
            s = step(cur, co)
            if s is None:
                break
            i, cur, co, canonical = s
            used.append(i)
            members.append((cur, co, max(0, -int(links[i]["gap_mode"])), fill[i] if canonical else rc(fill[i])))
        if cur < c:
            continue                    # the other end starts; it is visited first, so this is never reached with the path unmade
        for m in members:
            done.add(m[0])
        for i in used:
            link_path[i] = len(paths)
        paths.append(members)
    dec = ["J" if d is None else d for d in dec]
    return dec, paths, link_path


def path_name(names, path):
    return "%s_join%d" % (names[path[0][0]], len(path))


def joins_tsv(names, links, dec, at, res, paths, link_path):
    """joins.tsv: one line per returned link, no header"""
    by_link = dict(zip(at, res))
    out = []
    for i, k in enumerate(links):
        r = by_link.get(i)
        f = [names[int(k["a"])], "-" if int(k["info"]) & 1 else "+", names[int(k["b"])], "-" if int(k["info"]) & 2 else "+", int(k["reads"]), int(k["gap_mode"]), int(k["mode_reads"])]
        f += [int(r[n]) for n in ("columns", "matches", "fill_min", "fill_n")] if r is not None else [0, 0, 0, 0]
        f += [dec[i], path_name(names, paths[link_path[i]]) if dec[i] == "J" else "-"]
        out.append("\t".join(str(x) for x in f) + "\n")
    return "".join(out)


def joined_letters(contigs, path):
    out = []
    for c, o, trim, fill in path:
        s = contigs[c] if o == "+" else rc_bytes(contigs[c])
        out.append(fill + s[trim:])
    return "".join(out)


def joined_fasta(names, contigs, paths):
    """--joined: the contigs outside a path as they are, every path one record, ordered by the file index of the (start) contig"""
    start = {p[0][0]: p for p in paths}
    inside = {m[0] for p in paths for m in p}
    out = []
    for i, name in enumerate(names):
        if i in start:
            out.append(">%s\n%s\n" % (path_name(names, start[i]), joined_letters(contigs, start[i])))
        elif i not in inside:
            out.append(">%s\n%s\n" % (name, contigs[i]))
    return "".join(out)


def paths_tsv(names, contigs, paths):
    """--paths: joined_name ordinal name o start length trim fill, one line per member; ordinal and start are 1-based, length is the contig's"""
    out = []
    for p in paths:
        at = 0
        for n, (c, o, trim, fill) in enumerate(p):
            at += len(fill)
            out.append("\t".join(str(x) for x in (path_name(names, p), n + 1, names[c], o, at + 1, len(contigs[c]), trim, len(fill))) + "\n")
            at += len(contigs[c]) - trim
    return "".join(out)


def join(names, contigs, links, run_junctions, min_link_reads=2, overlap_percent=90):
    """the whole host chain; run_junctions(juncs) -> (res, letters).  -> dict(dec, paths, joins, joined, paths_tsv, juncs, res)"""
    lens = [len(s) for s in contigs]
    dec, juncs, at = first_decisions(links, lens, min_link_reads)
    res, letters = run_junctions(juncs)[:2] if len(juncs) else (np.zeros(0, RES_DTYPE), np.zeros(0, np.uint8))
    dec, paths, link_path = decide(links, lens, dec, at, res, letters, overlap_percent)
    return dict(dec=dec, paths=paths, juncs=juncs, res=res, joins=joins_tsv(names, links, dec, at, res, paths, link_path), joined=joined_fasta(names, contigs, paths),
                paths_tsv=paths_tsv(names, contigs, paths))
