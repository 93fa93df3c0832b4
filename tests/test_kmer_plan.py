"""kmermatcher's plan (carpedeam_amd/csrc/kmer_plan.h: which tuple layout a DB takes at each of the three entries, the equal-share cuts
of a histogram, the pass plan) against restatements of the code it replaced: the three layout ladders of cdm_kmermatch_ranks_impl,
cdm_kmermatch_part and cdm_kmermatch_split_begin, the two greedy cut loops of KmerJob::phaseA and kmermatchPassesT, and the P / B
arithmetic of kmermatchT, as they stood in kmermatch.hip before they were folded.  A different layout gives the same hits, only slower,
so no parity test notices a change of the choice; this one does.  CPU only: the header is plain arithmetic and compiles with g++."""
import itertools
import math
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu", "kmer_plan_driver.cpp")
SINGLE, PART, SPLIT = 0, 1, 2
LAYOUT_SWITCH = {None: 0, "wide": 1, "packed": 2, "slot": 3, "bogus": 4}
MAX_SEQ_LETTERS = 1 << 22


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kmer_plan") / "kmer_plan_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = r.stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


# ---------------------------------------------------------------------------------------------- the parent's code, restated
def bits_for(v):
    b = 1
    while (1 << b) < v:
        b += 1
    return b


def slots_per_seq(L, k):
    return L - k + 2 if L >= k else 1


def slot_layout_fits(n, max_len, residues, k):
    if n == 0 or residues != n * max_len or max_len < k:
        return False
    if 2 * k + 1 <= 27 or 2 * k - 9 > 31:
        return False
    if 2 * k + 1 + 2 * bits_for(max_len + 1) > 63:
        return False
    return n * slots_per_seq(max_len, k) < (1 << 32)


def packed_layout_fits(max_len, k):
    return 2 * k + 1 + 2 * bits_for(max_len + 1) <= 63


def one_pass_fits(n, residues, tot, bytes_per_slot):
    slots = residues + 2 * n
    if not tot:         # (hipMemGetInfo failed or reported nothing)
        return True
    return float(slots) * bytes_per_slot * 1.1 <= 0.80 * float(tot)


def needs_wide_key(n, max_len, env):
    return 2 * bits_for(n) + bits_for(2 * max_len + 2) + 1 > 63 or env["CDM_FORCE_WIDE_KEY"]


def ladder_16_bytes(n, max_len, force_huge):
    if max_len < 65535 and not force_huge:
        return "Wide"
    if max_len < (1 << 20) - 1 and n < (1 << 24) and not force_huge:
        return "Long"
    if max_len < MAX_SEQ_LETTERS:
        return "Huge"
    return "TooLong"


def parent_single(n, max_len, residues, k, tot, env, ranks):
    """cdm_kmermatch_ranks_impl"""
    fits = packed_layout_fits(max_len, k)
    packed = fits
    e = env["CDM_KMER_LAYOUT"]
    if e is not None:
        if e == "wide":
            packed = False
        elif e == "slot":
            pass
        elif e == "packed":
            if not fits:
                return "PackedUnfit"
        else:
            return "BadSwitch"
    want = e is None or e == "slot"
    if e == "slot" and not slot_layout_fits(n, max_len, residues, k):
        return "SlotUnfit"
    if (want and not ranks and slot_layout_fits(n, max_len, residues, k) and not env["CDM_KMER_SORT"] and not env["CDM_KMER_PASSES"]
            and one_pass_fits(n, residues, tot, 16.0 + 8.0)):
        return "Slot"
    if packed:
        return "Packed"
    return ladder_16_bytes(n, max_len, env["CDM_FORCE_HUGE_LAYOUT"])


def parent_part(n, max_len, residues, k, tot, env, ranks):
    """cdm_kmermatch_part with cdm_kmermatch_part_takes_slots"""
    lay = env["CDM_KMER_LAYOUT"]
    if ((lay is None or lay == "slot") and slot_layout_fits(n, max_len, residues, k) and one_pass_fits(n, residues, tot, 16.0 + 8.0)
            and not needs_wide_key(n, max_len, env)):
        return "Slot"
    if packed_layout_fits(max_len, k):
        return "Packed"
    return ladder_16_bytes(n, max_len, False)


def parent_split_begin(n, max_len, residues, k, tot, env, ranks):
    """cdm_kmermatch_split_begin"""
    if packed_layout_fits(max_len, k):
        return "Packed"
    return ladder_16_bytes(n, max_len, False)


def parent_cuts_phase_a(hh, nparts):
    """KmerJob::phaseA, head digits: nparts + 1 entries"""
    bins = len(hh)
    grand = sum(hh)
    cut = [0]
    target = (grand + nparts - 1) // nparts
    acc = 0
    for d in range(bins):
        if acc and acc + hh[d] > target and len(cut) < nparts:
            cut.append(d)
            acc = 0
        acc += hh[d]
    while len(cut) < nparts:
        cut.append(bins)
    cut.append(bins)
    return cut


def parent_cuts_passes(fine, P):
    """kmermatchPassesT, fine slices: the cuts, and P shrunk to the ranges that came out"""
    F = len(fine)
    grand = sum(fine)
    cut = [0]
    target = (grand + P - 1) // P
    acc = 0
    for f in range(F):
        if acc and acc + fine[f] > target and len(cut) < P:
            cut.append(f)
            acc = 0
        acc += fine[f]
    cut.append(F)
    return cut, len(cut) - 1


def parent_pass_plan(n, residues, tot, val_bytes):
    """kmermatchT without CDM_KMER_PASSES"""
    P = B = 1
    slots = residues + 2 * n
    if tot:
        one_pass, budget = float(slots) * (16.0 + 2.0 * val_bytes) * 1.1, 0.80 * float(tot)
        if one_pass > budget:
            P = int(min(255.0, math.ceil(float(slots) * (16.0 + 2.0 * val_bytes + 8.0) / (0.30 * float(tot)))))
            B = int(math.ceil(float(slots) * (32.0 + 4.0 * val_bytes + 16.0) / (0.30 * float(tot))))
    return P, B


# ---------------------------------------------------------------------------------------------- the tests
def test_layout_choice_of_the_three_entries(ask):
    k_values = (13, 14, 20, 21, 31)
    # 2^32 / 82 slots (100 letters, k = 20) lies between the last two: n x slots-per-sequence on each side of 2^32
    n_values = (1, (1 << 24) - 1, 1 << 24, 50_000_000, 52_377_649, 52_377_650)
    assert 52_377_649 * slots_per_seq(100, 20) < (1 << 32) <= 52_377_650 * slots_per_seq(100, 20)
    rows, want = [], []
    parents = {SINGLE: parent_single, PART: parent_part, SPLIT: parent_split_begin}
    switches = list(itertools.product(LAYOUT_SWITCH, (False, True), (False, True), (False, True), (False, True), (False, True)))
    for n, k in itertools.product(n_values, k_values):
        for max_len in (k - 1, k, 100, 65534, 65535, (1 << 20) - 2, (1 << 20) - 1, (1 << 22) - 1, 1 << 22):
            for residues in (n * max_len, n * max_len - 1):
                threshold = float(residues + 2 * n) * 24.0 * 1.1 / 0.80         # of the slot layout's one-pass check
                for tot in (0, int(threshold * 0.999), int(threshold * 1.001) + 1):
                    for lay, huge, wide_key, ksort, kpasses, ranks in switches:
                        env = {"CDM_KMER_LAYOUT": lay, "CDM_FORCE_HUGE_LAYOUT": huge, "CDM_FORCE_WIDE_KEY": wide_key, "CDM_KMER_SORT": ksort, "CDM_KMER_PASSES": kpasses}
                        for entry, parent in parents.items():
                            if entry != SINGLE and ranks:
                                continue        # (only the single-device entry is ever called over ranks)
                            rows.append("L %d %d %d %d %d %d %d %d %d %d %d %d" % (entry, n, max_len, residues, k, tot, LAYOUT_SWITCH[lay], huge, wide_key, ksort, kpasses, ranks))
                            want.append(parent(n, max_len, residues, k, tot, env, ranks))
    got = ask(rows)
    bad = [(r, g, w) for r, g, w in zip(rows, got, want) if g != w]
    assert not bad, "%d of %d rows differ, the first: %s" % (len(bad), len(rows), bad[:5])
    # the table reaches every outcome, and the slot layout on both entries that may take it
    assert set(want) == {"Slot", "Packed", "Wide", "Long", "Huge", "TooLong", "BadSwitch", "PackedUnfit", "SlotUnfit"}
    assert {r.split()[1] for r, w in zip(rows, want) if w == "Slot"} == {str(SINGLE), str(PART)}


def test_equal_share_cuts_against_both_loops(ask):
    rng = random.Random(20260117)
    cases = [([0] * 512, 4), ([0] * 511 + [977], 8), ([0] * 100 + [5] + [0] * 155, 3), ([3, 0, 0, 9] + [0] * 252, 16), ([1] * 256, 255), ([7], 1)]
    while len(cases) < 1000:
        bins = rng.choice((512, 256, 256, 64, 5))
        shape = rng.randrange(4)
        if shape == 0:
            h = [rng.randrange(1 << 40) for _ in range(bins)]
        elif shape == 1:        # a few heavy bins among light ones: equal slices of the k-mer space are anything but equal in tuples
            h = [rng.randrange(100) for _ in range(bins)]
            for _ in range(rng.randrange(1, 4)):
                h[rng.randrange(bins)] = rng.randrange(1 << 30)
        elif shape == 2:        # fewer non-empty bins than parts
            h = [0] * bins
            for _ in range(rng.randrange(1, 4)):
                h[rng.randrange(bins)] = rng.randrange(1, 1 << 20)
        else:
            h = [rng.randrange(3) for _ in range(bins)]
        cases.append((h, rng.choice((1, 2, 3, 4, 8, 16, 255, rng.randrange(1, 256)))))
    got = ask(["C %d %d %s" % (parts, len(h), " ".join(map(str, h))) for h, parts in cases])
    for (h, parts), line in zip(cases, got):
        cut = [int(x) for x in line.split()]
        want, shrunk = parent_cuts_passes(h, parts)
        assert cut == want and len(cut) - 1 == shrunk, (parts, h[:16], cut, want)
        padded = cut + [len(h)] * (parts + 1 - len(cut))          # (what phase A does with them)
        assert padded == parent_cuts_phase_a(h, parts), (parts, h[:16], padded)


def test_pass_plan(ask):
    GB = 1 << 30
    cases = []
    for slots, tot, val_bytes in itertools.product((1, 10_200_000, 5_100_000_000, 8_000_000_000, 27_000_000_000, 10 ** 13), (0, 16 * GB, 64 * GB, 192 * GB, 288 * GB), (4, 8)):
        for n in (1, slots // 102):
            cases.append((max(n, 0), slots - 2 * max(n, 0) if slots >= 2 * n else 0, tot, val_bytes))
    got = ask(["P %d %d %d %d" % c for c in cases])
    want = [parent_pass_plan(*c) for c in cases]
    assert [tuple(map(int, g.split())) for g in got] == want
    assert any(w == (1, 1) for w in want) and any(w[0] == 255 for w in want) and any(1 < w[0] < 255 for w in want)
