"""The device-resident sequence DB (carpedeam_amd/csrc/seqdb.hip) restated in numpy: from Python byte strings to the planes the
container holds, and the constructors that make one DB from another as list operations.  Test infrastructure: test_seqdb_model.py
checks it on hand-written rows, test_gpu_seqdb.py compares the device with it bit for bit.

Packing (k_pack): 16 letters per 32-bit code word, little end first, every sequence from a word boundary on.  A, C, G, T = 0..3.
'N' is code 0 plus a bit of the 16-bit mask half of its word.  Any other byte makes the sequence one with a raw row (hasN = 3): a
letter is mapped after toupper as NucleotideMatrix does (A; C M Y H -> C; G K B D V R S -> G; T U W -> T; every other letter is an
N: code 0 + mask bit), a byte that is no letter is an N as well.  hasN = 1 for a sequence whose only extras are 'N's, 0 for plain
ACGT.  A raw row holds the sequence's own bytes, 16 per code word; the DB has a raw plane iff a constructor gave it one."""
from collections import namedtuple

import numpy as np

DROP = 0xFFFFFFFF

Entry = namedtuple("Entry", "seq key ext raw")      # raw: the entry has a row of original letters (hasN bit 1)


class Db:
    def __init__(self, entries, raw_plane):
        self.entries, self.raw_plane = list(entries), bool(raw_plane)

    def __len__(self):
        return len(self.entries)


_CODE, _NBIT, _OTHER = np.zeros(256, np.uint32), np.ones(256, np.uint32), np.ones(256, np.uint32)
for _v, _letters in enumerate(("A", "CMYH", "GKBDVRS", "TUW")):
    for _c in _letters:
        for _b in (ord(_c), ord(_c) | 0x20):
            _CODE[_b], _NBIT[_b] = _v, 0
for _c in b"ACGTN":
    _OTHER[_c] = 0


def pack(seq):
    """-> code words, 16-bit mask halves, 'has a letter beyond ACGTN'"""
    b = np.frombuffer(bytes(seq), np.uint8)
    w = (b.size + 15) // 16
    pos = np.arange(b.size, dtype=np.uint32) & np.uint32(15)
    codes, mask = np.zeros(w, np.uint32), np.zeros(w, np.uint32)
    np.bitwise_or.at(codes, np.arange(b.size) >> 4, _CODE[b] << (np.uint32(2) * pos))
    np.bitwise_or.at(mask, np.arange(b.size) >> 4, _NBIT[b] << pos)
    return codes, mask.astype(np.uint16), bool(_OTHER[b].any())


def mapped(seq, with_mask=True):
    """the letters the packed form alone stands for"""
    b = np.frombuffer(bytes(seq), np.uint8)
    out = np.frombuffer(b"ACGT", np.uint8)[_CODE[b]]
    if with_mask:
        out = np.where(_NBIT[b] != 0, np.uint8(ord("N")), out)
    return out.astype(np.uint8).tobytes()


def text(e):
    """what a download gives for the entry"""
    return bytes(e.seq)


def upload(seqs, keys=None, ext=None):
    keys = list(range(len(seqs))) if keys is None else keys
    ext = [0] * len(seqs) if ext is None else ext
    entries = [Entry(bytes(s), int(k), int(x), pack(s)[2]) for s, k, x in zip(seqs, keys, ext)]
    return Db(entries, any(e.raw for e in entries))


def planes(db):
    n = len(db)
    lens = np.array([len(e.seq) for e in db.entries], np.uint32).reshape(n)
    woff = np.zeros(n + 1, np.uint32)
    woff[1:] = np.cumsum((lens.astype(np.uint64) + 15) // 16)
    packed = [pack(e.seq) for e in db.entries]
    has_n = np.array([3 if e.raw else (1 if p[1].any() else 0) for e, p in zip(db.entries, packed)], np.uint8).reshape(n)
    return {"woff": woff, "len": lens, "key": np.array([e.key for e in db.entries], np.uint32).reshape(n),
            "ext": np.array([e.ext for e in db.entries], np.uint8).reshape(n), "hasN": has_n,
            "codes": np.concatenate([p[0] for p in packed] + [np.zeros(0, np.uint32)]),
            "mask16": np.concatenate([p[1] for p in packed] + [np.zeros(0, np.uint16)]),
            "words": int(woff[n]), "residues": int(lens.sum(dtype=np.uint64)), "max_len": int(lens.max()) if n else 0}


def select(db, sel, ext_value=-1):
    """sel[i] = DROP drops entry i, any other value keeps its first sel[i] letters; ext_value < 0 carries the wasExtended flags.
    An entry with a raw row keeps the row (and hasN = 3) whatever the prefix still holds; an N flag follows the letters kept."""
    out = [Entry(e.seq[:int(t)], e.key, e.ext if ext_value < 0 else ext_value, e.raw) for e, t in zip(db.entries, sel) if int(t) != DROP]
    return Db(out, db.raw_plane)


def select_ext(db):
    return select(db, [len(e.seq) if e.ext == 1 else DROP for e in db.entries], 1)


def select_assembled(result, source, min_len):
    src = {e.key: len(e.seq) for e in source.entries}
    keep = lambda e: e.key in src and len(e.seq) > src[e.key] and len(e.seq) >= min_len
    return select(result, [len(e.seq) if keep(e) else DROP for e in result.entries], -1)


def overlay(base, grown, idx, ext):
    """base with entry idx[j] replaced by grown's entry j (letters and letter flags); keys are base's, ext the caller's"""
    src = list(base.entries)
    for j, i in enumerate(idx):
        src[int(i)] = grown.entries[j]
    return Db([Entry(s.seq, b.key, int(x), s.raw) for s, b, x in zip(src, base.entries, ext)], base.raw_plane or (grown is not None and grown.raw_plane))


def concat(a, b, ext_a, ext_b):
    parts = [(e, ext_a) for e in a.entries] + [(e, ext_b) for e in b.entries]
    return Db([Entry(e.seq, i, int(x), e.raw) for i, (e, x) in enumerate(parts)], a.raw_plane or b.raw_plane)


def from_packed(db, ext, with_mask=True, with_raw=False):
    """the DB rebuilt from its packed planes: ext one value or one per entry; without the raw plane the letters are the mapped ones,
    without the mask every N is an A"""
    ext = [ext] * len(db) if np.isscalar(ext) else ext
    if with_raw:
        return Db([Entry(e.seq, e.key, int(x), e.raw) for e, x in zip(db.entries, ext)], True)
    return Db([Entry(mapped(e.seq, with_mask), e.key, int(x), False) for e, x in zip(db.entries, ext)], False)
