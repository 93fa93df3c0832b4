#!/usr/bin/env python3
"""Generate tests/golden/fused/ from the reference's whole program (oracle/_ref/carpedeam_full, built by
`make -C oracle -f Makefile.ref`), on the CPU:

  calls_<case>.json   the call of `ancient_assemble` and every module call from `linclust` on (rmdb left out), logged behind a front
                      that routes by argv[0] as the product's front end does, paths replaced by $IN / $OUT / $TMP / $DAMAGE: what
                      `ancient_assemble_fused` derives its per-module parameter strings against (tests/test_fused_cli.py)
  <case>.fasta        the FASTA of the case, kept only if two runs with --threads 8 are byte-identical
  cases.json          per case: the arguments, the exit status, the size of the FASTA
  circ.reads.fa.gz    the reads of tests/golden/circ as FASTA

    python tests/golden/make_fused_golden.py
"""
import gzip
import json
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.path.join(ROOT, "oracle", "_ref", "carpedeam_full")
GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "fused")
sys.path.insert(0, ROOT)

# case -> (inputs relative to tests/golden, flags)
CASES = {
    "example": (["example/test_data.fq.gz"], []),
    "example_pairs_min30": (["mergereads/example.R1.fq.gz", "mergereads/example.R2.fq.gz"], ["--min-contig-len", "30"]),
    "example_pairs_default": (["mergereads/example.R1.fq.gz", "mergereads/example.R2.fq.gz"], []),
    "two": (["mergereads/two.A_R1.fq.gz", "mergereads/two.A_R2.fq.gz", "mergereads/two.B_R1.fq.gz", "mergereads/two.B_R2.fq.gz"], ["--min-contig-len", "30"]),
    "circ": (["fused/circ.reads.fa.gz"], ["--num-iter-reads-only", "3", "--num-iterations", "7", "--min-contig-len", "100"]),
    "example_flags": (["example/test_data.fq.gz"], ["--num-iterations", "8", "--num-iter-reads-only", "3", "--min-contig-len", "100", "--clust-min-seq-id", "0.95"]),
    # flags of which some reach linclust (CLUSTER_PAR: --zdrop, --clust-min-cov, --max-seq-len) and some do not (-e, --hash-shift, -v)
    "example_tail": (["example/test_data.fq.gz"], ["-e", "1e-05", "--hash-shift", "5", "-v", "2", "--zdrop", "40", "--clust-min-cov", "0.9", "--max-seq-len", "70000",
                                                   "--min-contig-len", "150"]),
}
LOGGED = ("example", "example_flags", "circ", "example_tail")      # the cases whose module calls are recorded
# where the FASTA of a case is kept (these two are goldens earlier makers wrote: verified here, not written again)
KEPT_ELSEWHERE = {"example": "example/ancient_assemble.fasta", "example_pairs_min30": "mergereads/example_ancient_assemble.fasta"}


def run(case, d, damage, log=None):
    inputs, flags = CASES[case]
    paths = [os.path.join(GOLD, p) for p in inputs]
    out, tmp = os.path.join(d, "out.fa"), os.path.join(d, "tmp")
    exe = REF
    if log:
        exe = os.path.join(d, "logwrap.sh")
        open(exe, "w").write('#!/bin/bash\nprintf "%%q " "$@" >> %s\necho >> %s\nexec -a %s %s "$@"\n' % (log, log, exe, REF))
        os.chmod(exe, 0o755)
    r = subprocess.run([exe, "ancient_assemble"] + paths + [out, tmp, "--ancient-damage", damage, "--threads", "8"] + flags, capture_output=True, text=True)
    return r, out, tmp, paths


def normalise(calls, paths, out, tmp, damage):
    """paths of a logged call -> placeholders; the workflow's hashed directory under tmp is part of $TMP"""
    hashed = None
    res = []
    for call in calls:
        norm = []
        for a in call:
            if hashed is None:
                m = re.match(re.escape(os.path.realpath(tmp)) + r"/(\d+)(/|$)", a)
                if m:
                    hashed = os.path.realpath(tmp) + "/" + m.group(1)
            for real, name in ((hashed, "$TMP"), (os.path.realpath(tmp), "$TMPDIR"), (tmp, "$TMPDIR"), (out, "$OUT"), (damage, "$DAMAGE")):
                if real and a.startswith(real):
                    a = name + a[len(real):]
            for i, p in enumerate(paths):
                if a == p:
                    a = "$IN%d" % i
            norm.append(a)
        res.append(norm)
    return res


def main():
    from carpedeam_amd import mmdb, synth
    os.makedirs(OUT, exist_ok=True)
    reads = mmdb.load_keyed(os.path.join(GOLD, "circ", "reads.keyed.gz"))
    fa = "".join(">r%d\n%s\n" % (k, reads[k][0].rstrip(b"\n").decode()) for k in sorted(reads))
    open(os.path.join(OUT, "circ.reads.fa.gz"), "wb").write(gzip.compress(fa.encode(), mtime=0))
    summary = {}
    with tempfile.TemporaryDirectory() as top:
        damage = os.path.join(top, "dhigh")
        synth.write_dhigh_profiles(damage)
        for case in CASES:
            runs = []
            for attempt in range(2):
                d = os.path.join(top, "%s_%d" % (case, attempt))
                os.makedirs(d)
                log = os.path.join(d, "calls.log") if (case in LOGGED and attempt == 0) else None
                r, out, tmp, paths = run(case, d, damage, log)
                data = open(out, "rb").read() if os.path.exists(out) else None
                runs.append((r.returncode, data))
                if log:
                    calls = normalise([shlex.split(l) for l in open(log) if l.strip()], paths, out, tmp, damage)
                    first = [i for i, c in enumerate(calls) if c[0] == "linclust"]
                    calls = calls[:1] + [c for c in calls[first[0]:] if c[0] != "rmdb"] if first else calls[:1]
                if attempt == 0:
                    tail = (r.stdout[-600:] + r.stderr[-600:]).strip().split("\n")[-3:]
            if runs[0] != runs[1]:
                print("%s: two runs differ - not kept" % case)
                continue
            if case in LOGGED:
                open(os.path.join(OUT, "calls_%s.json" % case), "w").write("[\n" + ",\n".join(json.dumps(c) for c in calls) + "\n]\n")
            status, data = runs[0]
            summary[case] = {"inputs": CASES[case][0], "flags": CASES[case][1], "exit_status": status, "fasta_bytes": None if data is None else len(data),
                             "records": None if data is None else data.count(b">")}
            if status != 0:
                summary[case]["last_output"] = tail
            if data is not None:
                if case in KEPT_ELSEWHERE:
                    assert data == open(os.path.join(GOLD, KEPT_ELSEWHERE[case]), "rb").read(), case + ": differs from the golden kept in " + KEPT_ELSEWHERE[case]
                    summary[case]["fasta"] = KEPT_ELSEWHERE[case]
                else:
                    open(os.path.join(OUT, case + ".fasta"), "wb").write(data)
                    summary[case]["fasta"] = "fused/" + case + ".fasta"
            print(case, summary[case])
        assert b"cycle:1" in open(os.path.join(OUT, "circ.fasta"), "rb").read(), "circ: no circular contig reached createhdb"
    json.dump(summary, open(os.path.join(OUT, "cases.json"), "w"), indent=1, sort_keys=True)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
