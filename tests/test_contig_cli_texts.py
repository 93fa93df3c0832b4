"""The six contig_* commands and ancient_assemble_fused without a device: the complete text and the exit status of every usage
line and refusal, against tests/golden/contig_cli_texts.json.  The other flag tests look for substrings; this one pins every byte of
stderr (its `Time for processing` line left out), so that work on the commands' host code cannot reword, reorder or drop a message.
The fixture was recorded from the binary of the commit named in its first entry and is never rewritten from the code under test."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carpedeam_amd", "carpedeam_mi355x")
GOLDEN = os.path.join(ROOT, "tests", "golden", "contig_cli_texts.json")

IO = ["contigs.fa", "reads.fq", "out"]
GAP = ["--gapped", "--gap-band", "--gap-min-columns"]
# per command: the positional arguments and [flag, below its range, above it] of every ranged flag (GAP stands for the three gapped flags)
RANGED = {
    "contig_damage": [["--damage-ends", "0", "65"]],
    "contig_depth": [["--depth-edge", "-1", "1048577"], GAP],
    "contig_variants": [["--mask-ends", "-1", "65"], ["--min-depth", "0", "1000001"], ["--min-alt-count", "0", "1000001"], ["--min-alt-percent", "-1", "101"], GAP],
    "contig_breaks": [["--break-anchor", "0", "1025"], ["--break-edge", "0", "1048577"], ["--min-span", "0", "1000001"], ["--min-span-percent", "-1", "101"],
                      ["--min-piece", "0", "1048577"], GAP],
    "contig_map": [["--primary-only", "-1", "2"], GAP],
    "contig_indels": [["--min-depth", "0", "1000001"], ["--min-indel-count", "0", "1000001"], ["--min-indel-percent", "-1", "101"], ["--gap-band", "0", "32"],
                      ["--gap-min-columns", "0", "4097"]],
    "ancient_assemble_fused": [["--damage-ends", "0", "65"], ["--depth-edge", "-1", "1048577"], ["--mask-ends", "-1", "65"], ["--min-depth", "0", "1000001"],
                               ["--min-alt-count", "0", "1000001"], ["--min-alt-percent", "-1", "101"], ["--break-anchor", "0", "1025"], ["--break-edge", "0", "1048577"],
                               ["--min-span", "0", "1000001"], ["--min-span-percent", "-1", "101"]],
}


def cases():
    out = []
    for module, ranged in RANGED.items():
        fused = module == "ancient_assemble_fused"
        io = ["reads.fq", "out.fa", "tmp"] if fused else IO
        out.append([module, io[0]])                                 # a wrong number of arguments
        out.append([module] if fused else [module] + io[:2])
        out.append([module] + io + ["--no-such-flag", "1"])
        for r in ranged:
            if r is GAP:
                out += [[module] + io + f for f in (["--gapped", "-1"], ["--gapped", "2"], ["--gapped", "1", "--gap-band", "0"], ["--gapped", "1", "--gap-band", "32"],
                                                   ["--gapped", "1", "--gap-min-columns", "0"], ["--gapped", "1", "--gap-min-columns", "4097"],
                                                   ["--gap-band", "8"], ["--gap-min-columns", "32"], ["--gapped", "0", "--gap-band", "8"], ["--gapped", "0", "--gap-min-columns", "32"])]
            else:
                out += [[module] + io + [r[0], v] for v in r[1:]]
        if "--break-edge" in [r[0] for r in ranged]:
            out.append([module] + io + ["--break-edge", "10"])      # below --break-anchor's default
            out.append([module] + io + ["--break-edge", "100", "--break-anchor", "101"])
    out.append(["contig_depth", "contigs.fa", "a.fq", "b.fq", "out", "--depth-track", "out.bg"])
    out.append(["contig_depth", "contigs.fa", "a.fq", "b.fq", "c.fq", "out", "--depth-track", "out.bg", "--gapped", "1"])
    out += [["contig_map"] + IO + ["--read-group", g] for g in ("", "a\tb")]
    out += [["contig_damage"] + IO + ["--gapped", "1"], ["contig_indels"] + IO + ["--gapped", "1"], ["contig_variants"] + IO + ["extra"], ["contig_map"] + IO + ["extra"]]
    # ancient_assemble_fused's own checks around the reports' flags
    out += [["ancient_assemble_fused", "a.fq", "b.fq", "c.fq", "out.fa", "tmp"], ["ancient_assemble_fused", "reads.fq", "out.fa", "tmp", "--variant-sites", "s.tsv"],
            ["ancient_assemble_fused", "reads.fq", "out.fa", "tmp", "-k", "20"], ["ancient_assemble_fused", "reads.fq", "out.fa", "tmp", "--cov-mode", "0"],
            ["ancient_assemble_fused", "reads.fq", "out.fa", "a tmp"]]
    return out


CASES = cases()


def run(args, cwd):
    e = {k: v for k, v in os.environ.items() if k not in ("CARPEDEAM_REF_BIN", "CDM_TIMING", "CDM_FUSED_DRY_RUN")}
    # (no device is needed for any of these; where a machine has some, they are hidden, so that a check that came too late would show)
    e.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([EXE] + args, capture_output=True, text=True, env=e, cwd=cwd, timeout=120)
    return r.returncode, "".join(l for l in r.stderr.splitlines(True) if not l.startswith("Time for processing")), r.stdout


@pytest.fixture(scope="module", autouse=True)
def built():
    from carpedeam_amd import build
    build.build()


@pytest.fixture(scope="module")
def golden():
    entries = json.load(open(GOLDEN))
    assert "recorded_from" in entries[0]
    return {json.dumps(e["args"]): e for e in entries[1:]}


def test_the_fixture_holds_every_case_once(golden):
    assert sorted(golden) == sorted(json.dumps(c) for c in CASES) and len(golden) == len(CASES)
    # every command is refused with both statuses, and the usage lines are there
    for module in RANGED:
        mine = [e for e in golden.values() if e["args"][0] == module]
        assert {e["status"] for e in mine} == {1, 77} and any(e["stderr"].startswith("Usage: carpedeam " + module) for e in mine), module


@pytest.mark.parametrize("args", CASES, ids=lambda a: " ".join(a).replace("\t", "\\t") or "none")
def test_status_and_text(args, golden, tmp_path):
    want = golden[json.dumps(args)]
    status, stderr, stdout = run(args, str(tmp_path))
    assert (status, stderr, stdout) == (want["status"], want["stderr"], "")
    assert os.listdir(tmp_path) == []         # refused before anything is written
