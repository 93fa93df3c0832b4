#!/usr/bin/env python3
"""tests/golden/rescore_directed/: what the reference's own object code (oracle/_ref/carpedeam_ref rescorediagonal, built by
`make -C oracle -f Makefile.ref`) makes of the case sets of tests/rescorecases.py, under every parameter row of every set.

    python tests/golden/make_rescore_directed.py

Writes, per set, one <row>.keyed.gz - the alignment DB's text - and digest.txt: a digest of the generator's inputs (sequences,
hits, group names, flags) and the number of groups.  Data only: the inputs are regenerated from the seed at test time, and
tests/test_rescore_directed.py holds the digest to what it regenerated.  A group for which the reference ends on a signal has
undefined behaviour there: the script stops and names the set and the row, the group has to leave the generator
(rescorecases.DROPPED).
"""
import gzip
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from carpedeam_amd import mmdb  # noqa: E402
import rescorecases  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "carpedeam_ref")


def gz_write(path, text):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(text.encode("latin1"))


def main(exe=REF, out=rescorecases.DIR):
    if not os.path.exists(exe):
        sys.exit("build oracle/_ref first: make -C oracle -f Makefile.ref")
    with tempfile.TemporaryDirectory() as tmp:
        for name, make in rescorecases.SETS:
            S = make()
            d = os.path.join(out, name)
            os.makedirs(d, exist_ok=True)
            p = lambda s: os.path.join(tmp, name + "_" + s)
            S.write(p("db"), p("pref"))
            total = 0
            for row, par in S.rows:
                r = subprocess.run([exe, "rescorediagonal", p("db"), p("db"), p("pref"), p(row)] + par.flags() + ["--threads", "1"], capture_output=True, text=True)
                if r.returncode:
                    sys.exit("reference %s on set %s, row %s: %s" % ("ended with signal %d" % -r.returncode if r.returncode < 0 else "failed", name, row, r.stderr[-2000:]))
                assert mmdb.read_dbtype(p(row)) == mmdb.DBTYPE_ALIGNMENT_RES
                gz_write(os.path.join(d, row + ".keyed.gz"), mmdb.dump_keyed(p(row)))
                total += len(rescorecases.records(mmdb.read_db(p(row))))
            with open(os.path.join(d, "digest.txt"), "w") as f:
                f.write("%s %d\n" % (S.digest(), len(S.groups)))
            print("%s: %d sequences, %d groups, %d rows, %d records" % (name, len(S.seqs), len(S.groups), len(S.rows), total))


if __name__ == "__main__":
    main(*sys.argv[1:3])
