"""A CPU restatement of `mergereads` (FLASH's pair merging with mergereads' fixed parameters), written from the contract in
include/carpedeam_hip.h (cdm_pairs_merge): the oracle of the device kernel in the GPU tests, itself checked against the reference's
outputs (tests/golden/mergereads) by tests/test_mergereads.py.

Floats are numpy float32, as the reference computes density and quality score; qualities are the raw ASCII bytes."""
import hashlib
import struct

import numpy as np

MIN_OVERLAP, MAX_OVERLAP, MAX_DENSITY = 15, 65, np.float32(0.10)

# FLASH's complement table: IUPAC codes and lower case to their complements, U -> A, every other byte '.'
_PAIRS = {"A": "T", "B": "V", "C": "G", "D": "H", "G": "C", "H": "D", "K": "M", "M": "K", "N": "N", "R": "Y", "S": "S", "T": "A",
          "U": "A", "V": "B", "W": "W", "Y": "R"}
COMP = bytearray(b"." * 256)
for _k, _v in _PAIRS.items():
    COMP[ord(_k)] = ord(_v)
    COMP[ord(_k.lower())] = ord(_v.lower())
COMP = bytes(COMP)


def revcomp(seq, qual):
    return bytes(seq.translate(COMP)[::-1]), bytes(qual[::-1])


def best_shift(s1, q1, s2, q2, min_ov=MIN_OVERLAP, max_ov=MAX_OVERLAP, max_dens=MAX_DENSITY):
    """s2 / q2 already reverse-complemented.  The shift of R2 against R1, or None."""
    L1, L2 = len(s1), len(s2)
    max_dens = np.float32(max_dens)
    best_d, best_q, best_i = max_dens + np.float32(1.0), np.float32(0.0), None
    a1 = np.frombuffer(s1, np.uint8)
    a2 = np.frombuffer(s2, np.uint8)
    b1 = np.frombuffer(q1, np.uint8).astype(np.int64)
    b2 = np.frombuffer(q2, np.uint8).astype(np.int64)
    N = ord("N")
    for i in range(max(0, L1 - L2), L1 - min_ov + 1):
        n = L1 - i
        x, y = a1[i:], a2[:n]
        called = (x != N) & (y != N)
        ov = int(called.sum())
        if ov < min_ov:
            continue
        mis = called & (x != y)
        mm = int(mis.sum())
        qs = int(np.minimum(b1[i:], b2[:n])[mis].sum())
        sl = np.float32(min(ov, max_ov))
        q, d = np.float32(qs) / sl, np.float32(mm) / sl
        if d <= best_d and (d < best_d or q < best_q):
            best_d, best_q, best_i = d, q, i
    if best_i is None or best_d > max_dens:
        return None
    return best_i


def combine(s1, q1, s2, q2, b):
    L1 = len(s1)
    out = bytearray(s1[:b])
    for k in range(b, L1):
        x, y, qx, qy = s1[k], s2[k - b], q1[k], q2[k - b]
        if x == y or qx > qy:
            out.append(x)
        elif qx < qy:
            out.append(y)
        else:
            out.append(x if y == ord("N") else y)
    out += s2[L1 - b:]
    return bytes(out)


def merge_pair(r1, r2, **kw):
    """r1, r2: (name, seq, qual) as read.  Returns the entries [(name, seq)] mergereads writes for the pair."""
    (n1, s1, q1), (n2, s2, q2) = r1, r2
    if any(c >= 0x80 for c in q1 + q2):
        raise ValueError("quality byte >= 0x80")
    t2, u2 = revcomp(s2, q2)
    b = best_shift(s1, q1, t2, u2, **kw)
    if b is None:
        return [(n1, s1), (n2, t2)]
    return [(n1, combine(s1, q1, t2, u2, b))]


def read_fastq(path):
    """Well-formed four-line FASTQ[.gz] as kseq reads it for these fixtures: (name, seq, qual); a record whose quality has the wrong
    length ends the file."""
    import gzip
    data = open(path, "rb").read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    lines = data.split(b"\n")
    recs = []
    for k in range(0, len(lines) - 3, 4):
        h, s, _, q = lines[k:k + 4]
        if len(q) != len(s):
            break
        recs.append((h[1:].split()[0] if h[1:].split() else b"", s, q))
    return recs


def mergereads(file_pairs):
    """[(R1 path, R2 path), ...] -> the entries [(name, seq)] in key order."""
    entries = []
    for p1, p2 in file_pairs:
        for r1, r2 in zip(read_fastq(p1), read_fastq(p2)):
            entries += merge_pair(r1, r2)
    return entries


def db_files(entries):
    """The files mergereads writes for these entries: {suffix: bytes} (data, .index, .dbtype, _h, _h.index, _h.dbtype)."""
    out = {}
    for suffix, payloads, dbtype in (("", [s + b"\n" for _, s in entries], 1), ("_h", [n + b"\n" for n, _ in entries], 12)):
        data, index, off = bytearray(), [], 0
        for k, p in enumerate(payloads):
            data += p + b"\0"
            index.append(b"%d\t%d\t%d\t1\n" % (k, off, len(p) + 1))
            off += len(p) + 1
        out[suffix] = bytes(data)
        out[suffix + ".index"] = b"".join(index)
        out[suffix + ".dbtype"] = struct.pack("<i", dbtype)
    return out


def digests(files):
    return {k: hashlib.sha256(v).hexdigest() for k, v in files.items()}
