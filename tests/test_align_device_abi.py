"""The device path of `align` at the drop-in boundary, checked without a GPU: cdm_align_hits / cdm_align_mode are declared, exported and
bound, the POD records have the header's layout, CDM_ALIGN=device without a device fails loudly, and CDM_ALIGN=host is what the module
does on a small input when the switch is left alone."""
import ctypes
import os
import re
import subprocess

import pytest

from carpedeam_amd import mmdb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
FLAGS = ("-a 0 --alignment-mode 2 --alignment-output-mode 0 --wrapped-scoring 1 -e 0.001 --min-seq-id 0.9 --min-aln-len 0 --seq-id-mode 0 --alt-ali 0 -c 0.8 --cov-mode 1 "
         "--max-seq-len 200000 --max-rejected 2147483647 --max-accept 2147483647 --gap-open 5 --gap-extend 2 --zdrop 200 --threads 1 --compressed 0 -v 0").split()


@pytest.fixture(scope="module")
def libpath():
    from carpedeam_amd import build
    return build.build()


def small_db(tmp_path):
    import numpy as np
    rng = np.random.default_rng(11)
    base = "".join("ACGT"[i] for i in rng.integers(0, 4, 500))
    var = base[:200] + "T" + base[200:350] + base[353:]
    var = var[:40] + ("A" if var[40] != "A" else "C") + var[41:]
    mmdb.write_seqdb(str(tmp_path / "db"), [base, var, base[20:480]])
    pref = [(0, b"0\t100\t0\n1\t100\t0\n2\t100\t20\n"), (1, b"1\t100\t0\n0\t100\t0\n"), (2, b"2\t100\t0\n0\t100\t-20\n")]
    mmdb.write_db(str(tmp_path / "pref"), pref, mmdb.DBTYPE_PREFILTER_REV_RES)
    return str(tmp_path / "db"), str(tmp_path / "pref")


def run(tmp_path, out, mode):
    db, pref = small_db(tmp_path)
    env = dict(os.environ, CDM_TIMING="1")
    env.pop("CDM_ALIGN", None)
    if mode:
        env["CDM_ALIGN"] = mode
    return subprocess.run([EXE, "align", db, db, pref, str(tmp_path / out)] + FLAGS, capture_output=True, text=True, env=env)


def test_symbols_declared_exported_and_bound(libpath):
    from carpedeam_amd import capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "carpedeam_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(libpath)
    for name in ("cdm_align_hits", "cdm_align_mode"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert capi.lib().cdm_align_hits.argtypes is not None


def test_record_layouts_match_header():
    from carpedeam_amd import capi
    assert ctypes.sizeof(capi.AlignParams) == 16 and ctypes.sizeof(capi.AlignHit) == 28
    assert capi.ALIGN_HIT_DTYPE.itemsize == 28 and capi.ALIGN_RESULT_DTYPE.itemsize == 32
    assert [capi.ALIGN_HIT_DTYPE.fields[f][1] for f in ("query", "target", "q_len", "t_len", "q_end", "t_end", "reverse", "wrapped", "stale_q", "stale_t")] == [0, 4, 8, 12, 16, 20, 24, 25, 26, 27]
    header = open(os.path.join(ROOT, "include", "carpedeam_hip.h")).read()
    body = re.search(r"typedef struct cdm_align_result \{(.*?)\} cdm_align_result;", header, re.S).group(1)
    names = re.findall(r"\b([a-z_]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == list(capi.ALIGN_RESULT_DTYPE.names)


def test_switch_values(libpath):
    from carpedeam_amd import capi
    old = os.environ.get("CDM_ALIGN")
    try:
        for value, want in (("host", 1), ("device", 2), (None, 0)):
            if value is None:
                os.environ.pop("CDM_ALIGN", None)
            else:
                os.environ["CDM_ALIGN"] = value
            assert capi.lib().cdm_align_mode() == want
        os.environ["CDM_ALIGN"] = "gpu"
        assert capi.lib().cdm_align_mode() < 0 and b"CDM_ALIGN" in capi.lib().cdm_last_error()
    finally:
        if old is None:
            os.environ.pop("CDM_ALIGN", None)
        else:
            os.environ["CDM_ALIGN"] = old
        capi.lib()


def test_device_path_without_a_device_fails_loudly(libpath, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = run(tmp_path, "dev", "device")
    assert r.returncode != 0
    assert "no CPU fallback" in r.stderr and "device" in r.stderr
    assert not os.path.exists(str(tmp_path / "dev.index"))


def test_host_and_default_agree_without_a_device(libpath, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    a, b = run(tmp_path, "host", "host"), run(tmp_path, "auto", None)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr[-800:], b.stderr[-800:])
    assert "align: path=host" in a.stderr and "align: path=host" in b.stderr
    host, auto = mmdb.read_db(str(tmp_path / "host")), mmdb.read_db(str(tmp_path / "auto"))
    assert host == auto and sum(v[0].count(b"\n") for v in host.values()) >= 5
    assert mmdb.read_dbtype(str(tmp_path / "host")) == mmdb.read_dbtype(str(tmp_path / "auto")) == mmdb.DBTYPE_ALIGNMENT_RES
