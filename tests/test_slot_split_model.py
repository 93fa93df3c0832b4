"""The slot layout's split of sort 1 (round 9): how many of the 2k k-mer bits the global radix passes leave to the grouping kernel.
cdm_kmer_slot_split answers without a device, through the argument check that cdm_kmermatch runs on the same switch."""
import pytest

from carpedeam_amd import capi

RADIX_BITS = 9      # csrc/radix.h rx::BITS


@pytest.fixture(autouse=True)
def no_switch(monkeypatch):
    monkeypatch.delenv("CDM_SLOT_LOWBITS", raising=False)


def served(k, n):
    """what the passes take: at most two 9-bit passes behind the head digit (the grouping kernel's sort word - 8 bits of bucket ordinal,
    n, 9 of position, in 32 bits up to n = 15 and in 64 beyond - holds every such n: checked here, never a reason to refuse)"""
    rem = 2 * k - RADIX_BITS - n
    ok = n >= 0 and 0 <= rem <= 2 * RADIX_BITS
    assert not ok or 8 + n + 9 <= (32 if n <= 15 else 64)
    return ok


@pytest.mark.parametrize("k", range(14, 21))
def test_default_split_sorts_27_kmer_bits_globally(k):
    n = capi.kmer_slot_split(k)
    assert n == max(0, 2 * k - 27)
    assert served(k, n)
    assert 2 * k - n == min(2 * k, 27)          # the head digit and two full passes
    assert n < 2 * k + 1 - 27 or k < 14         # one bit fewer than the split of the 12-byte layouts, whose 27 include the unused-slot bit


@pytest.mark.parametrize("k", (4, 13, 21, 31))
def test_split_is_refused_for_a_k_the_layout_does_not_take(k):
    with pytest.raises(capi.CdmError):
        capi.kmer_slot_split(k)


@pytest.mark.parametrize("k", (14, 17, 20))
def test_switch_is_taken_inside_its_bounds_and_refused_outside(monkeypatch, k):
    lo, hi = 2 * k - 9 - 18, 2 * k - 9          # 0 <= 2k - 9 - n <= 18
    for n in range(-2, 2 * k + 2):
        monkeypatch.setenv("CDM_SLOT_LOWBITS", str(n))
        if max(lo, 0) <= n <= hi:
            assert served(k, n)
            assert capi.kmer_slot_split(k) == n
        else:
            assert not served(k, n)
            with pytest.raises(capi.CdmError) as e:
                capi.kmer_slot_split(k)
            assert "CDM_SLOT_LOWBITS" in str(e.value)
    # the split of the rounds before 9 stays reachable for A/B runs
    monkeypatch.setenv("CDM_SLOT_LOWBITS", str(2 * k + 1 - 27))
    assert capi.kmer_slot_split(k) == 2 * k + 1 - 27


@pytest.mark.parametrize("bad", ("", "x", "13x", "1e3", "99999999999999999999"))
def test_switch_must_be_a_number(monkeypatch, bad):
    monkeypatch.setenv("CDM_SLOT_LOWBITS", bad)
    with pytest.raises(capi.CdmError):
        capi.kmer_slot_split(20)
