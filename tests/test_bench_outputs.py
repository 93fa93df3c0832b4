"""bench.py --dump-outputs: what the last timed step computed, as .npy files - float arrays, at most 64 MB, keyed (the same arrays
whatever order a build hands the records back in), and the same from run to run of the same command."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class FakeDb:
    """stands in for capi.SeqDb: meta() and download_into() on host arrays"""

    def __init__(self, lens, keys, ext, seqs):
        self.lens, self.keys, self.ext, self.seqs = lens, keys, ext, seqs

    @classmethod
    def random(cls, n, seed):
        rng = np.random.default_rng(seed)
        lens = rng.integers(0, 300, n).astype(np.uint32)
        seqs = [rng.choice(np.frombuffer(b"ACGTN", np.uint8), int(l)).tobytes() for l in lens]
        return cls(lens, rng.permutation(n).astype(np.uint32), rng.integers(0, 2, n).astype(np.uint8), seqs)

    def permuted(self, seed):
        p = np.random.default_rng(seed).permutation(len(self.lens))
        return FakeDb(self.lens[p], self.keys[p], self.ext[p], [self.seqs[i] for i in p])

    def meta(self):
        return self.lens, self.keys, self.ext

    def download_into(self, buf, offs):
        for o, s in zip(offs, self.seqs):
            buf[int(o):int(o) + len(s)] = np.frombuffer(s, np.uint8)
            buf[int(o) + len(s)] = ord("\n")


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.fixture
def bench(monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", os.environ.get("OMP_NUM_THREADS", "16"))     # (bench.py sets a default at import: undone after the test)
    import bench
    return bench


@pytest.mark.parametrize("n", [0, 7, 100_000])
def test_dump_seqdb_sample_is_keyed_and_bounded(bench, tmp_path, n):
    db = FakeDb.random(n, 1)
    bench.dump_seqdb(str(tmp_path / "a"), "asm", db, (11, 12))
    bench.dump_seqdb(str(tmp_path / "b"), "asm", db.permuted(5), (11, 12))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["asm_" + k for k in ("counts", "extended", "keys", "length_hist", "lengths", "letters", "offsets")]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert list(a["asm_counts"]) == [n, int(db.lens.sum()), int(db.ext.sum()), 11, 12]
    assert a["asm_length_hist"].sum() == n
    by_key = {int(k): (s, int(e)) for k, s, e in zip(db.keys, db.seqs, db.ext)}
    keys, offs = a["asm_keys"], a["asm_offsets"].astype(np.int64)
    assert np.all(np.diff(keys) > 0)
    if n <= bench.DUMP_SAMPLE:
        assert len(keys) == n
    else:
        assert bench.DUMP_SAMPLE // 2 < len(keys) <= bench.DUMP_SAMPLE
    for i, k in enumerate(keys):
        s, e = by_key[int(k)]
        assert a["asm_letters"][offs[i]:offs[i + 1]].astype(np.uint8).tobytes() == s
        assert a["asm_lengths"][i] == len(s) and a["asm_extended"][i] == e


@pytest.mark.gpu
def test_bench_dump_outputs_repeat(tmp_path):
    """two plain runs of the same command: the result line says what it timed, and the dumps are equal array for array"""
    lines, dumps = [], []
    for run in ("a", "b"):
        d = str(tmp_path / run)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--reads", "200000", "--dump-outputs", d],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
        out = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
        assert len(out) == 1, r.stdout[-1500:]
        lines.append(json.loads(out[0]))
        dumps.append(_load(d))
    for line in lines:
        assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert "cpu_baseline" not in line           # (--full only)
    a, b = dumps
    assert sorted(a) == sorted(b) and "asm_letters" in a
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    counts = a["asm_counts"]
    assert counts[0] == 200000 and counts[1] > 200000 * 100
    assert (counts[3], counts[4]) == (lines[0]["config"]["prefilter_hits"], lines[0]["config"]["alignments"])
    assert len(a["asm_keys"]) > 10000
