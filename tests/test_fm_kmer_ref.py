"""Host side of the k-mer correction, no GPU: debwt_fm_weak_trials (api.weak_trials) against the reference of kmer_ref.py
on random masks and on the named shapes, its errors and capacity return; and the conditions on the seeded read set that
the GPU comparison relies on -- the reference alone meets every case, and it removes the errors it is meant to remove."""
import ctypes

import numpy as np
import pytest

import kmer_ref as KR


def got_trials(counts, k, min_count):
    from debwt_amd import api
    return [tuple(int(x) for x in t) for t in api.weak_trials(counts, k, min_count).tolist()]


def test_weak_trials_random_masks():
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(20000):
        k, nk = int(rng.integers(1, 7)), int(rng.integers(1, 15))
        counts = (rng.random(nk) < rng.random()).astype(np.uint32) * 5
        want = KR.trials(counts.tolist(), k, 3)
        assert got_trials(counts, k, 3) == want, (k, counts)
        seen.add(len(want))
    assert {0, 1, 2, 3, 4} <= seen


def mask(nk, *runs):
    c = np.full(nk, 9, dtype=np.uint32)
    for a, b in runs:
        c[a:b + 1] = 1
    return c


def test_weak_trials_named_shapes():
    k = 5
    # an interior run of exactly k: both trials; of k - 1: left alone; of 2k + 3: both
    assert got_trials(mask(20, (4, 8)), k, 3) == [(4, 8, 8, 4, 0), (4, 8, 8, 8, 1)]
    assert got_trials(mask(20, (4, 7)), k, 3) == []
    assert got_trials(mask(30, (4, 16)), k, 3) == [(4, 16, 8, 4, 0), (4, 16, 16, 16, 1)]
    # touching the left end: the right trial alone, however short; the right end: the left trial alone
    assert got_trials(mask(20, (0, 1)), k, 3) == [(0, 1, 1, 1, 1)]
    assert got_trials(mask(20, (17, 19)), k, 3) == [(17, 19, 21, 17, 0)]
    # both ends: no trial; nk = 1; no weak k-mer; two runs
    assert got_trials(mask(20, (0, 19)), k, 3) == []
    assert got_trials(mask(1, (0, 0)), k, 3) == [] and got_trials(mask(1), k, 3) == []
    assert got_trials(mask(20), k, 3) == []
    assert got_trials(mask(30, (0, 2), (10, 14)), k, 3) == [(0, 2, 2, 2, 1), (10, 14, 14, 10, 0), (10, 14, 14, 14, 1)]
    for c in (mask(20, (4, 8)), mask(30, (0, 2), (10, 14), (28, 29))):
        assert got_trials(c, k, 3) == KR.trials(c.tolist(), k, 3)
    # the threshold: counts[j] < min_count
    c = np.array([3, 2, 2, 3, 3, 3], dtype=np.uint32)
    assert got_trials(c, 2, 3) == [(1, 2, 2, 1, 0), (1, 2, 2, 2, 1)] and got_trials(c, 2, 2) == []


def test_weak_trials_errors_and_capacity():
    from debwt_amd import _lib, api
    L = _lib.lib()
    c = mask(30, (0, 2), (10, 14))
    p = c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    out = (_lib.DebwtFmTrial * 4)()
    assert L.debwt_fm_weak_trials(p, len(c), 0, 3, out, 4) == -1
    assert L.debwt_fm_weak_trials(p, len(c), 5, 0, out, 4) == -1
    assert L.debwt_fm_weak_trials(p, len(c), 5, 3, None, 1) == -1
    with pytest.raises(api.DebwtError):
        api.weak_trials(c, 0, 3)
    # the return is the number of trials; only `capacity` of them are written
    assert L.debwt_fm_weak_trials(p, len(c), 5, 3, None, 0) == 3
    assert L.debwt_fm_weak_trials(p, len(c), 5, 3, out, 2) == 3
    assert (out[1].run_a, out[1].pos, out[1].kind) == (10, 14, 0) and (out[2].run_a, out[2].pos, out[2].window) == (0, 0, 0)
    assert L.debwt_fm_weak_trials(p, len(c), 5, 3, out, 4) == 3 and (out[2].run_a, out[2].pos, out[2].kind) == (10, 14, 1)
    assert L.debwt_fm_weak_trials(None, 0, 5, 3, out, 4) == 0


def test_correct_defaults():
    from debwt_amd import _lib
    o = _lib.DebwtFmCorrectOpts(k=7, min_count=0, max_rounds=0, flags=0)
    _lib.lib().debwt_fm_correct_defaults(ctypes.byref(o))
    assert (o.k, o.min_count, o.max_rounds, o.flags) == (0, 3, 4, 1)


def test_read_set_holds_every_case():
    """at k = 15, min_count 3, both strands, 4 rounds the reference alone meets each case the GPU comparison is to cover"""
    k = 15
    S = KR.read_set()
    q = KR.correction_queries(k)
    res = KR.corrected(k, 3, True, 4)
    n = len(S["records"])
    assert 90_000 < sum(len(s) for s in S["records"]) < 110_000
    assert {r[1] for r in res} == {KR.SHORT, KR.CLEAN, KR.FIXED, KR.WEAK}
    fixes = [(i, nt) for i, r in enumerate(res) for nt in r[5] if nt[0] == "fix"]
    assert {nt[2] for _, nt in fixes} == {KR.LEFT, KR.RIGHT}
    assert any(nt[3] < k - 1 for _, nt in fixes) and any(nt[3] > len(q[i]) - k for i, nt in fixes)
    assert any(nt[1] >= 1 for _, nt in fixes)                                          # a read that needs a second round
    short, empty, with_n, snp, foreign, lower, two, left_end, right_end, clean_lower = range(n, n + 10)
    assert res[short][1] == KR.SHORT and res[empty][1] == KR.SHORT and res[short][0] == q[short]
    g = S["genome"]
    assert "N" in q[with_n] and res[with_n][0] == g[300:370] and res[with_n][1] == KR.FIXED
    assert ("two", 0) in res[snp][5] and res[snp][1] == KR.WEAK and res[snp][0] == q[snp]
    assert res[foreign][3] == len(q[foreign]) - k + 1 and res[foreign][2] == 0 and res[foreign][1] == KR.WEAK
    # the case of untouched bytes is kept: one upper-case letter, the fix, in a lower-case read
    assert res[lower][0].upper() == g[400:470] and sum(c.isupper() for c in res[lower][0]) == 1
    diff = [j for j in range(80) if q[two][j] != g[500 + j]]
    assert len(diff) == 2 and diff[1] - diff[0] < k and res[two][0] == g[500:580] and res[two][2] == 2
    assert res[left_end][0] == g[600:670] and res[right_end][0] == g[700:770]
    assert res[clean_lower] == (g[800:870].lower(), KR.CLEAN, 0, 0, 0, [])
    # one round is not enough for every read
    one = KR.corrected(k, 3, True, 1)
    assert any(a[0] != b[0] for a, b in zip(one, res))


def test_reference_removes_the_errors():
    """at k = 15, min_count 3, both strands, 4 rounds: of the injected wrong bases at most 5 % stay, and at least 90 % of
    the reads that had one are FIXED (a prototype of the rules went from 983 wrong bases to 9, 720 of 731 reads FIXED)"""
    S = KR.read_set()
    res = KR.corrected(15, 3, True, 4)
    wrong = lambda a, b: sum(x != y for x, y in zip(a, b))                             # noqa: E731
    before = after = bad_reads = fixed = 0
    for i in range(1500):
        w = wrong(S["records"][i], S["truth"][i])
        before += w
        after += wrong(res[i][0], S["truth"][i])
        if w:
            bad_reads += 1
            fixed += res[i][1] == KR.FIXED
    print(f"wrong bases {before} -> {after}; erroneous reads {bad_reads}, FIXED {fixed}")
    assert before > 800 and after <= 0.05 * before and fixed >= 0.9 * bad_reads
