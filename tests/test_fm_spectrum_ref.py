"""Definition 9 without a GPU: debwt_fm_spectrum_threshold (host code of the library, through ctypes and
api.spectrum_threshold) against the Python rule of spectrum_ref.py on crafted histograms, the reference values of the
seeded read set, the two identities of the totals on every geometry case, and a self-check that the chosen inputs tell
a reference without the palindrome rule, or with k-mers across separators, from the right one."""
import ctypes

import numpy as np
import pytest

import fm_definition as F
import kmer_ref as KR
import spectrum_ref as SR

EINVAL = -1
CASES = F.geometry_cases()


def lib_threshold(hist, total, nbins=None):
    from debwt_amd import _lib
    L = _lib.lib()
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    out = _lib.DebwtFmSpectrumSummary()
    rc = L.debwt_fm_spectrum_threshold(h.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(h) if nbins is None else nbins,
                                       int(total), ctypes.byref(out))
    return rc, (int(out.valley), int(out.peak), int(out.est_size))


def total_of(hist):
    return sum(c * h for c, h in enumerate(hist))


CRAFTED = {
    "monotone": ([0, 90, 70, 50, 30, 10, 5, 0], (0, 0, 0)),
    "flat": ([0, 7, 7, 7, 7, 7, 7, 7], (0, 0, 0)),
    "rise_at_1": ([0, 5, 9, 4, 1, 0, 0, 0], (1, 2, None)),
    "valley_3_peak_6": ([0, 50, 20, 4, 9, 30, 41, 33, 12, 3, 0, 2], (3, 6, None)),
    "plateau_before_rise": ([0, 50, 8, 8, 8, 20, 30, 10, 0, 0], (4, 6, None)),
    "peak_tie_takes_smallest": ([0, 40, 3, 25, 10, 25, 25, 1, 0], (2, 3, None)),
    "second_hump_higher": ([0, 40, 3, 10, 5, 2, 30, 4, 0], (2, 6, None)),
    "overflow_higher_than_peak": ([0, 40, 3, 10, 5, 2, 1, 1, 999], (2, 3, None)),
    "rise_only_into_overflow": ([0, 40, 30, 20, 10, 5, 4, 3, 999], (0, 0, 0)),
    "rise_at_last_inner_bin": ([0, 40, 30, 20, 10, 5, 4, 6, 1], (6, 7, None)),
    "all_zero": ([0] * 16, (0, 0, 0)),
    "nbins_2": ([0, 12], (0, 0, 0)),
    "nbins_3": ([0, 3, 12], (0, 0, 0)),
    "nbins_4": ([0, 3, 12, 1], (1, 2, None)),
}


@pytest.mark.parametrize("name", list(CRAFTED))
def test_threshold_on_crafted_histograms(name):
    from debwt_amd import api
    hist, (valley, peak, est) = CRAFTED[name]
    total = total_of(hist) + 1000 * hist[-1]                     # the overflow bin stands for larger multiplicities
    want = SR.threshold(hist, total)
    assert want[:2] == (valley, peak)
    if est is None:
        est = (total - sum(c * hist[c] for c in range(valley))) // peak
    assert want[2] == est
    rc, got = lib_threshold(hist, total)
    assert rc == 0 and got == want
    assert api.spectrum_threshold(hist, total) == {"valley": valley, "peak": peak, "est_size": est}


def test_threshold_on_random_histograms():
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(400):
        nbins = int(rng.integers(2, 40))
        hist = rng.integers(0, 6, nbins).tolist()
        hist[0] = 0
        if rng.integers(0, 2):
            hist = [0] + sorted(hist[1:], reverse=True)
        total = total_of(hist)
        want = SR.threshold(hist, total)
        assert lib_threshold(hist, total) == (0, want)
        seen.add(want[0] > 0)
    assert seen == {True, False}


def test_threshold_errors():
    from debwt_amd import _lib, api
    L = _lib.lib()
    h = np.zeros(4097, dtype=np.uint64)
    out = _lib.DebwtFmSpectrumSummary()
    p = h.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert L.debwt_fm_spectrum_threshold(None, 8, 0, ctypes.byref(out)) == EINVAL
    assert L.debwt_fm_spectrum_threshold(p, 8, 0, None) == EINVAL
    for nbins in (0, 1, 4097):
        assert L.debwt_fm_spectrum_threshold(p, nbins, 0, ctypes.byref(out)) == EINVAL
    assert L.debwt_fm_spectrum_threshold(p, 4096, 0, ctypes.byref(out)) == 0
    assert L.debwt_fm_spectrum_threshold(p, 2, 0, ctypes.byref(out)) == 0
    with pytest.raises(api.DebwtError):
        api.spectrum_threshold([0], 0)


def test_kmer_string():
    from debwt_amd import api
    assert api.kmer_string(0, 1) == "A" and api.kmer_string(3, 1) == "T"
    assert api.kmer_string(0b00011011, 4) == "ACGT"
    assert api.kmer_string(4 ** 32 - 1, 32) == "T" * 32 and api.kmer_string(1 << 62, 32) == "C" + "A" * 31
    rng = np.random.default_rng(3)
    for k in (1, 5, 31, 32):
        w = KR.rand_dna(rng, k)
        assert api.kmer_string(SR.code_of(w), k) == w == SR.string_of(SR.code_of(w), k)
    for code, k in ((4, 1), (0, 0), (0, 33), (-1, 3)):
        with pytest.raises(ValueError):
            api.kmer_string(code, k)


@pytest.mark.parametrize("k,both,valley,peak", [(15, True, 6, 22), (21, True, 5, 19), (31, True, 3, 13), (15, False, 3, 9),
                                                (1, True, 0, 0), (1, False, 0, 0)])
def test_read_set_reference_values(k, both, valley, peak):
    D = SR.of_read_set(k, both)
    hist = SR.histogram(D, 256)
    distinct, total, over = SR.totals(D, 256)
    assert sum(hist) == distinct and hist[0] == 0
    want = SR.threshold(hist, total)
    assert want[:2] == (valley, peak)
    assert lib_threshold(hist, total) == (0, want)


def test_read_set_size_estimate():
    """the genome is 3,000 b plus a 200 b second haplotype; measured 3109..3236"""
    for k in (11, 15, 16, 21, 31, 32):
        D = SR.of_read_set(k, True)
        hist = SR.histogram(D, 256)
        rc, (valley, peak, est) = lib_threshold(hist, SR.totals(D, 256)[1])
        assert rc == 0 and valley > 0 and 2700 <= est <= 3300, (k, valley, peak, est)


def check_identities(strs, k):
    fwd, both = SR.members(strs, k, False), SR.members(strs, k, True)
    assert SR.totals(fwd, 256)[1] == SR.forward_total(strs, k)
    assert SR.totals(both, 256)[1] == SR.forward_total(strs, k) + SR.palindrome_occ(strs, k)
    for D in (fwd, both):
        for nbins in (2, 3, 256):
            hist = SR.histogram(D, nbins)
            distinct, total, over = SR.totals(D, nbins)
            assert sum(hist) == distinct == len(D) and hist[0] == 0
            assert total - over == sum(c * hist[c] for c in range(nbins - 1))
    return SR.palindrome_occ(strs, k)


@pytest.mark.parametrize("name", list(CASES))
def test_total_identities_on_geometry_cases(name):
    strs = F.strings(CASES[name])
    for k in (1, 2, 3, 4, 8, 32):
        check_identities(strs, k)


def test_total_identities_on_the_read_set():
    strs = KR.read_set()["records"]
    pal = {k: check_identities(strs, k) for k in (1, 4, 15, 16, 21, 32)}
    assert pal[4] > 0 and pal[16] > 0 and pal[1] == pal[15] == pal[21] == 0      # odd k has no such k-mer
    assert len(CASES) == 25


def test_inputs_tell_wrong_references_apart():
    """a reference that counts a k-mer equal to its reverse complement once, or that admits k-mers across separators,
    differs from the right one on the inputs the GPU tests use"""
    strs = KR.read_set()["records"]
    for k in (4, 16):
        assert SR.members(strs, k, True, palindromes_twice=False) != SR.of_read_set(k, True)
    for k in (4, 21, 32):
        for both in (False, True):
            assert SR.members(strs, k, both, across_separators=True) != SR.of_read_set(k, both)
    for name in ("all_T_x3", "T_ones_400", "ones_600", "dup_40x20"):
        s = F.strings(CASES[name])
        assert SR.members(s, 2, False, across_separators=True) != SR.members(s, 2, False), name
    s = F.strings(CASES["all_T_x3"])                                # "AA".."TT": T^k with A^k, never its own
    assert SR.members(s, 2, True) == {SR.code_of("AA"): 399 + 36}
    assert SR.members(F.strings(CASES["ones_600"]), 2, True) == {}
