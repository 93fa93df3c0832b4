"""The numpy model of the sequence DB container (seqdb_model.py) on hand-written rows: no device."""
import numpy as np
import pytest

import seqdb_model as M

# (letters, code words, 16-bit mask halves, hasN)
ROWS = [
    (b"", [], [], 0),
    (b"A", [0x0], [0x0], 0),
    (b"ACGT", [0xE4], [0x0], 0),
    (b"TTTTTTTTTTTTTTTT", [0xFFFFFFFF], [0x0], 0),
    (b"ACGTACGTACGTACGTC", [0xE4E4E4E4, 0x1], [0x0, 0x0], 0),
    (b"N", [0x0], [0x1], 1),
    (b"TNT", [0x33], [0x2], 1),
    (b"AAAAAAAAAAAAAAANNG", [0x0, 0x8], [0x8000, 0x1], 1),
    (b"acgt", [0xE4], [0x0], 3),
    (b"MYH", [0x15], [0x0], 3),             # -> C
    (b"KBDVRS", [0xAAA], [0x0], 3),         # -> G
    (b"UWuw", [0xFF], [0x0], 3),            # -> T
    (b"CnXx-*Ec", [0x4001], [0x7E], 3),     # n, X, bytes that are no letter, letters without a base: N
]


@pytest.mark.parametrize("seq,codes,mask,has_n", ROWS, ids=[r[0].decode() or "empty" for r in ROWS])
def test_pack_rows(seq, codes, mask, has_n):
    c, m, other = M.pack(seq)
    assert c.tolist() == codes and m.tolist() == mask and c.dtype == np.uint32 and m.dtype == np.uint16
    assert other == (has_n == 3)
    p = M.planes(M.upload([seq]))
    assert p["hasN"].tolist() == [has_n] and p["woff"].tolist() == [0, len(codes)] and p["len"].tolist() == [len(seq)]


def test_planes_of_a_db():
    db = M.upload([r[0] for r in ROWS], keys=range(10, 10 + len(ROWS)), ext=[i & 1 for i in range(len(ROWS))])
    p = M.planes(db)
    assert p["woff"].tolist() == [0, 0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14] and p["words"] == 14
    assert p["codes"].tolist() == sum((r[1] for r in ROWS), []) and p["mask16"].tolist() == sum((r[2] for r in ROWS), [])
    assert p["residues"] == sum(len(r[0]) for r in ROWS) and p["max_len"] == 18
    assert p["key"][0] == 10 and p["ext"].tolist() == [i & 1 for i in range(len(ROWS))]
    assert db.raw_plane and not M.upload([b"ACGT", b"NN"]).raw_plane
    assert M.planes(M.Db([], False))["woff"].tolist() == [0]


def test_mapped_letters():
    assert M.mapped(b"acgtRYKMSWBDHVUnX-") == b"ACGTGCGCGTGGCGTNNN"
    assert M.mapped(b"ANnC", with_mask=False) == b"AAAC"


def test_select_keeps_order_prefixes_and_letter_flags():
    db = M.upload([b"ACGTN", b"ACGTNA", b"AcGT", b"GG"], keys=[3, 5, 8, 9], ext=[1, 0, 1, 0])
    out = M.select(db, [4, 5, 1, M.DROP], -1)
    assert [(e.seq, e.key, e.ext) for e in out.entries] == [(b"ACGT", 3, 1), (b"ACGTN", 5, 0), (b"A", 8, 1)]
    assert M.planes(out)["hasN"].tolist() == [0, 1, 3]       # the N dropped, the N kept, the raw row stays a raw row
    assert out.raw_plane and [e.ext for e in M.select(db, [0, 0, 0, 0], 0).entries] == [0, 0, 0, 0]
    assert len(M.select(db, [M.DROP] * 4, 1)) == 0 and M.select(db, [M.DROP] * 4, 1).raw_plane
    assert [e.key for e in M.select_ext(db).entries] == [3, 8]
    src = M.upload([b"ACG", b"ACGTNA", b"A"], keys=[3, 5, 7])
    assert [e.key for e in M.select_assembled(db, src, 0).entries] == [3]        # 5 did not grow, 8 and 9 are not in the source
    assert [e.key for e in M.select_assembled(db, src, 6).entries] == []


def test_overlay_concat_and_from_packed():
    base = M.upload([b"AAAA", b"CCNC", b"GG"], keys=[1, 2, 4])
    grown = M.upload([b"GGt", b"T" * 17], keys=[0, 1])
    out = M.overlay(base, grown, [2, 0], [1, 0, 1])
    assert [(e.seq, e.key, e.ext) for e in out.entries] == [(b"T" * 17, 1, 1), (b"CCNC", 2, 0), (b"GGt", 4, 1)]
    assert M.planes(out)["hasN"].tolist() == [0, 1, 3] and out.raw_plane and not base.raw_plane
    same = M.overlay(base, None, [], [0, 0, 0])
    assert [e.seq for e in same.entries] == [e.seq for e in base.entries] and not same.raw_plane
    cat = M.concat(base, grown, 0, 1)
    assert [(e.key, e.ext) for e in cat.entries] == [(0, 0), (1, 0), (2, 0), (3, 1), (4, 1)] and cat.raw_plane
    assert M.planes(cat)["woff"].tolist() == [0, 1, 2, 3, 4, 6]
    back = M.from_packed(out, 1)
    assert [e.seq for e in back.entries] == [b"T" * 17, b"CCNC", b"GGT"] and M.planes(back)["hasN"].tolist() == [0, 1, 0] and not back.raw_plane
    assert np.array_equal(M.planes(back)["codes"], M.planes(out)["codes"])
    assert [e.seq for e in M.from_packed(out, [0, 1, 0], with_mask=False).entries][1] == b"CCAC"
    assert [e.raw for e in M.from_packed(out, 0, with_raw=True).entries] == [False, False, True]
