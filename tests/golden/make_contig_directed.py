#!/usr/bin/env python3
"""tests/golden/contig_directed/: the case sets of tests/contigcases.py and what the reference's own object code
(oracle/_ref/carpedeam_ref ancient_contig_merge, built by `make -C oracle -f Makefile.ref`) makes of them.

    python tests/golden/make_contig_directed.py

Writes corr.keyed.gz, aln.keyed.gz and cmerge.keyed.gz under one directory per set (--unsafe 0; the maxlen set under its own
--max-seq-len).  Data only: the generator's inputs and the reference binary's outputs.  A group for which the reference ends on a
signal has undefined behaviour there: the script stops and names the set, the group has to leave the generator.
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
import contigcases  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "carpedeam_ref")
OUT = contigcases.DIR


def gz_write(path, text):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(text.encode("latin1"))


def main(exe=REF):
    if not os.path.exists(exe):
        sys.exit("build oracle/_ref first: make -C oracle -f Makefile.ref")
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "dhigh")
        synth.write_dhigh_profiles(prefix)
        for name, make, max_seq_len in contigcases.SETS:
            S = make()
            d = os.path.join(OUT, name)
            os.makedirs(d, exist_ok=True)
            p = lambda s: os.path.join(tmp, name + "_" + s)
            mmdb.write_from_keyed(p("corr"), S.seq_keyed(), mmdb.DBTYPE_NUCLEOTIDES)
            mmdb.write_from_keyed(p("aln"), S.aln_keyed(), mmdb.DBTYPE_ALIGNMENT_RES)
            r = subprocess.run([exe, "ancient_contig_merge", p("corr"), p("aln"), p("cmerge")] + contigcases.flags_for(max_seq_len) +
                               ["--ancient-damage", prefix, "--threads", "4"], capture_output=True, text=True)
            if r.returncode:
                sys.exit("reference %s on set %s: %s" % ("ended with signal %d" % -r.returncode if r.returncode < 0 else "failed", name, r.stderr[-2000:]))
            for s in ("corr", "aln", "cmerge"):
                gz_write(os.path.join(d, s + ".keyed.gz"), mmdb.dump_keyed(p(s)))
            out = mmdb.canon(mmdb.read_db(p("cmerge")))
            got = [contigcases.sides(S, g, *out[g["key"]])[0] for g in S.groups]
            sizes = [os.path.getsize(os.path.join(d, s + ".keyed.gz")) for s in ("corr", "aln", "cmerge")]
            print("%s: %d sequences, %d groups, %d records, %d queries extended, files of %s bytes" % (
                name, len(S.seqs), len(S.groups), S.total_records(), sum(x != "none" for x in got), sizes))


if __name__ == "__main__":
    main(*sys.argv[1:2])
