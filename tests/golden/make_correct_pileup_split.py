#!/usr/bin/env python3
"""tests/golden/correct_pileup_split/: the case set of tests/test_gpu_correct_pileup_split.py and what the reference's own object
code (oracle/_ref/carpedeam_ref ancient_correction, built by `make -C oracle -f Makefile.ref`) makes of it.

    python tests/golden/make_correct_pileup_split.py

Writes reads.keyed.gz, aln_0.keyed.gz and corr_0.keyed.gz.  Data only: the generator's inputs and the reference binary's output."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "carpedeam_amd"))
from carpedeam_amd import mmdb, synth  # noqa: E402
from carpedeam_amd.stageflags import A_FLAGS  # noqa: E402
from make_correct_directed import gz_write  # noqa: E402
import test_gpu_correct_pileup_split as cases  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "carpedeam_ref")
OUT = os.path.join(ROOT, "tests", "golden", "correct_pileup_split")


def main(exe=REF):
    if not os.path.exists(exe):
        sys.exit("build oracle/_ref first: make -C oracle -f Makefile.ref")
    S, _ = cases.build_cases()
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        p = lambda s: os.path.join(tmp, s)
        synth.write_dhigh_profiles(p("dhigh"))
        mmdb.write_from_keyed(p("in"), S.seq_keyed(), mmdb.DBTYPE_NUCLEOTIDES)
        mmdb.write_from_keyed(p("aln"), S.aln_keyed(), mmdb.DBTYPE_ALIGNMENT_RES)
        r = subprocess.run([exe, "ancient_correction", p("in"), p("aln"), p("corr")] + list(A_FLAGS) + ["--ancient-damage", p("dhigh"), "--threads", "4"],
                           capture_output=True, text=True)
        if r.returncode:
            sys.exit("reference %s: %s" % ("ended with signal %d" % -r.returncode if r.returncode < 0 else "failed", r.stderr[-2000:]))
        for s, fn in (("in", "reads"), ("aln", "aln_0"), ("corr", "corr_0")):
            gz_write(os.path.join(OUT, fn + ".keyed.gz"), mmdb.dump_keyed(p(s)))
        corr = mmdb.canon(mmdb.read_db(p("corr")))
        changed = sum(corr[g["query"]][0] != S.seqs[g["query"]] for g in S.groups)
        print("%d sequences, %d groups, %d records, %d queries changed" % (len(S.seqs), len(S.groups), sum(len(v) for v in S.recs.values()), changed))


if __name__ == "__main__":
    main(*sys.argv[1:2])
