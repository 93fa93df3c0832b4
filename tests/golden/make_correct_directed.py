#!/usr/bin/env python3
"""tests/golden/correct_directed/: the case sets of tests/correctcases.py and what the reference's own object code
(oracle/_ref/carpedeam_ref ancient_correction, built by `make -C oracle -f Makefile.ref`) makes of them.

    python tests/golden/make_correct_directed.py

Writes reads.keyed.gz, aln_0.keyed.gz and corr_0.keyed.gz for the main set (the layout of the other data sets) and the same three
files under lonely/ and single/.  Data only: the generator's inputs and the reference binary's outputs.  A group for which the
reference ends on a signal has undefined behaviour there: the script stops and names the set, the group has to leave the generator.
"""
import gzip
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from carpedeam_amd import mmdb, synth  # noqa: E402
from carpedeam_amd.stageflags import A_FLAGS  # noqa: E402
import correctcases  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "carpedeam_ref")
OUT = os.path.join(ROOT, "tests", "golden", "correct_directed")


def gz_write(path, text):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(text.encode("latin1"))


def main(exe=REF):
    if not os.path.exists(exe):
        sys.exit("build oracle/_ref first: make -C oracle -f Makefile.ref")
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "dhigh")
        synth.write_dhigh_profiles(prefix)
        for name, make in correctcases.SETS:
            S = make()
            d = OUT if name == "main" else os.path.join(OUT, name)
            os.makedirs(d, exist_ok=True)
            p = lambda s: os.path.join(tmp, name + "_" + s)
            mmdb.write_from_keyed(p("in"), S.seq_keyed(), mmdb.DBTYPE_NUCLEOTIDES)
            mmdb.write_from_keyed(p("aln"), S.aln_keyed(), mmdb.DBTYPE_ALIGNMENT_RES)
            r = subprocess.run([exe, "ancient_correction", p("in"), p("aln"), p("corr")] + list(A_FLAGS) + ["--ancient-damage", prefix, "--threads", "4"],
                               capture_output=True, text=True)
            if r.returncode:
                sys.exit("reference %s on set %s: %s" % ("ended with signal %d" % -r.returncode if r.returncode < 0 else "failed", name, r.stderr[-2000:]))
            for s, fn in (("in", "reads"), ("aln", "aln_0"), ("corr", "corr_0")):
                gz_write(os.path.join(d, fn + ".keyed.gz"), mmdb.dump_keyed(p(s)))
            corr, src = mmdb.read_db(p("corr")), S.seq_keyed()
            changed = sum(mmdb.canon(corr)[g["query"]][0] != src[g["query"]][0].rstrip(b"\n") for g in S.groups)
            print("%s: %d sequences, %d groups, %d records, %d queries changed" % (name, len(S.seqs), len(S.groups), sum(len(v) for v in S.recs.values()), changed))


if __name__ == "__main__":
    main(*sys.argv[1:2])
