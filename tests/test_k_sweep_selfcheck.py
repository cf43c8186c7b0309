"""The comparisons of tests/test_k_sweep_gpu.py run on the CPU: fed what the oracle and the definition give, every check
passes; fed one hand-made wrong value -- the red array or the SP symbols of k + 1, sorted keys with two neighbours swapped,
a distinct key missing, a BWT with two unequal rows swapped, a '#' row, the '$' row, a stat of k + 1, a k-mer count, a
counter that stayed 0 where the rule says the form ran (and one that rose where it cannot run), a hash -- the check that
looks at it fails.  No GPU and no library call.  Also here: the rule of radix_split as restated there against the facts
the existing sort tests state, the range cut against the cap, and the keys of the stand-alone sorts against their contract."""
import numpy as np
import pytest

import k_ladder as KL
import test_k_sweep_gpu as T

K = 16


@pytest.fixture(scope="module")
def E(oracle):
    return KL.expected("small")


def _fails(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


def _swap_unequal_rows(words):
    """the packed rows with two neighbouring rows of different symbols swapped (rows 2j, 2j + 1 of one word)"""
    w = words.copy()
    for i in range(len(w)):
        x = int(w[i])
        for s in range(0, 62, 2):
            a, b = (x >> s) & 3, (x >> (s + 2)) & 3
            if a != b:
                w[i] = np.uint64((x & ~(0xF << s)) | (b << s) | (a << (s + 2)))
                return w
    raise AssertionError("every word holds one symbol")


def test_a_f_keys(E):
    want = KL.sorted_keys("small", K)
    T.check_keys(want.copy(), np.unique(want), want)
    i = int(np.flatnonzero(want[1:] != want[:-1])[0])
    bad = want.copy()
    bad[[i, i + 1]] = bad[[i + 1, i]]
    _fails(T.check_keys, bad, np.unique(want), want)
    _fails(T.check_keys, want.copy(), np.unique(want)[:-1], want)
    _fails(T.check_keys, KL.sorted_keys("small", K + 1), np.unique(want), want)


def test_a_d_stage_arrays(E):
    T.check_stage_arrays(E, K, E.red[K].copy(), E.sp[K].copy())
    assert not np.array_equal(E.red[K], E.red[K + 1]) or not np.array_equal(E.sp[K], E.sp[K + 1])
    for k in KL.KS[:-1]:                                         # a kernel one K off, at every k
        _fails(T.check_stage_arrays, E, k, E.red[k + 1], E.sp[k + 1])
        _fails(T.check_stage_arrays, E, k + 1, E.red[k], E.sp[k])
    sp = E.sp[K].copy()
    sp[len(sp) // 2] ^= 1
    _fails(T.check_stage_arrays, E, K, E.red[K], sp)


def test_a_e_g_stats(E):
    T.check_stats(E, K, dict(E.stats[K]))
    assert E.stats[K]["special_branch_num"] != E.stats[K + 1]["special_branch_num"]
    _fails(T.check_stats, E, K, dict(E.stats[K + 1]), ("special_branch_num",))
    for nm in T.STAT_NAMES:
        _fails(T.check_stats, E, K, dict(E.stats[K], **{nm: E.stats[K][nm] + 1}))


def test_result(E):
    T.check_result(E, E.words.copy(), E.hrows.copy(), E.drow, E.rows.copy())
    _fails(T.check_result, E, _swap_unequal_rows(E.words), E.hrows, E.drow)
    h = E.hrows.copy()
    h[3] += np.uint64(1)
    _fails(T.check_result, E, E.words, h, E.drow)
    _fails(T.check_result, E, E.words, E.hrows, E.drow + 1)
    rows = E.rows.copy()
    i = int(np.flatnonzero(rows[1:] != rows[:-1])[0])
    rows[[i, i + 1]] = rows[[i + 1, i]]
    _fails(T.check_result, E, E.words, E.hrows, E.drow, rows)


def test_kmer_counts(E, oracle):
    km, ct = oracle.kmer_count(E.sym, K)
    T.check_kmer_counts((km.copy(), ct.copy()), (km, ct))
    bad = ct.copy()
    bad[0] += np.uint64(1)
    _fails(T.check_kmer_counts, (km, bad), (km, ct))
    _fails(T.check_kmer_counts, oracle.kmer_count(E.sym, K + 1), (km, ct))


def test_b_c_counters():
    env = {"DEBWT_PREFIX_DIGITS": "2", "DEBWT_BUCKET_PASS": "1"}
    want = T.expected_sort_counters("small", 20, None, env, 3)
    assert want == {"stat_bucket_passes": 1, "bucket_passes": (">=", 1), "low_finishes": (">=", 1)}
    T.check_counters(want, {"stat_bucket_passes": 1, "bucket_passes": 2, "low_finishes": 1, "pair_passes": 5})
    _fails(T.check_counters, want, {"stat_bucket_passes": 1, "bucket_passes": 0, "low_finishes": 1})
    _fails(T.check_counters, want, {"stat_bucket_passes": 0, "bucket_passes": 1, "low_finishes": 1})
    _fails(T.check_counters, want, {"stat_bucket_passes": 1, "bucket_passes": 1, "low_finishes": 0})
    # k = 12 with three digits: 24 - 24 < 1, nothing of the hybrid sort may run
    want = T.expected_sort_counters("small", 12, None, {"DEBWT_PREFIX_DIGITS": "3", "DEBWT_BUCKET_PASS": "1"}, 3)
    assert want == {"stat_bucket_passes": 0, "bucket_passes": 0, "low_finishes": 0}
    _fails(T.check_counters, want, {"stat_bucket_passes": 0, "bucket_passes": 1, "low_finishes": 0})
    _fails(T.check_counters, want, {"stat_bucket_passes": 0, "bucket_passes": 0, "low_finishes": 1})
    want = T.expected_sort_counters("small", 20, None, {"DEBWT_HIST_EVERY_PASS": "1"}, 3)
    _fails(T.check_counters, want, {"stat_bucket_passes": 0, "bucket_passes": 0, "low_finishes": 1, "pair_passes": 1})


def test_radix_split_restated_against_stated_facts():
    """tests/test_gpu_finish_low_words.py: one digit of a 40-bit key cuts at bit 32, of a 34-bit key at bit 26 (low-word
    form); four digits of 64 bits cut at bit 32, one digit at bit 56 (whole keys); DEBWT_FINISH_LOW=0 takes the whole-key
    form.  tests/test_gpu_bucket_pass.py: a forced sort of up to 2^22 keys has two prefix digits.  radix_sort.h: not hybrid
    when key_bits - 8 T < 1; by default the bucket pass serves key ranges of four digits; DEBWT_BUCKET_PASS=1 gives every
    sort two prefix digits at least."""
    S = T.radix_split
    assert S(1000, 40, 3, False, {"DEBWT_PREFIX_DIGITS": "1"}) == {"T": 1, "pshift": 32, "bucket": False, "low": True}
    assert S(1000, 34, 3, False, {"DEBWT_PREFIX_DIGITS": "1"})["pshift"] == 26
    assert S(100, 64, 3, False, {"DEBWT_PREFIX_DIGITS": "4"}) == {"T": 4, "pshift": 32, "bucket": False, "low": True}
    assert S(100, 64, 3, False, {"DEBWT_PREFIX_DIGITS": "1"}) == {"T": 1, "pshift": 56, "bucket": False, "low": False}
    assert not S(1000, 40, 3, False, {"DEBWT_PREFIX_DIGITS": "1", "DEBWT_FINISH_LOW": "0"})["low"]
    # (a digit more as soon as a bucket would hold more than 64 keys on average, n >> 8 T > 64: 2^14 keys have one digit
    # still, 65 * 2^8 two; 65 * 2^16 three)
    assert S(1 << 14, 64, 3, False, {})["T"] == 1 and S(65 << 8, 64, 3, True, {})["T"] == 2
    assert S(1 << 22, 64, 3, True, {"DEBWT_BUCKET_PASS": "1"})["T"] == 2 and S(65 << 16, 64, 3, True, {"DEBWT_BUCKET_PASS": "1"})["T"] == 3
    assert S(2, 64, 3, True, {"DEBWT_BUCKET_PASS": "1"}) == {"T": 2, "pshift": 48, "bucket": True, "low": False}
    assert S(100, 24, 3, False, {"DEBWT_PREFIX_DIGITS": "3"}) is None and S(100, 32, 3, False, {"DEBWT_PREFIX_DIGITS": "4"}) is None
    assert S(100, 26, 3, False, {"DEBWT_PREFIX_DIGITS": "3"})["pshift"] == 2
    assert S(1 << 20, 64, 1, False, {}) is None
    assert S(100, 64, 3, True, {"DEBWT_PREFIX_DIGITS": "4"})["bucket"] and not S(100, 64, 3, False, {"DEBWT_PREFIX_DIGITS": "4"})["bucket"]
    assert not S(100, 64, 3, True, {"DEBWT_PREFIX_DIGITS": "4", "DEBWT_BUCKET_PASS": "0"})["bucket"]
    assert not S(100, 64, 3, True, {"DEBWT_PREFIX_DIGITS": "1", "DEBWT_BUCKET_PASS": "1"})["bucket"]


@pytest.mark.parametrize("k", (12, 13, 25, 32))
def test_range_cut(k):
    total = len(KL.sorted_keys("mid", k))
    assert T.range_sizes("mid", k, None) == [total]
    for cap in (4096, 20000):
        sizes = T.range_sizes("mid", k, cap)
        assert sum(sizes) == total and len(sizes) >= -(-total // cap) and all(sizes)
        assert sum(1 for m in sizes if m > cap) <= 2, sizes      # only a single bin above the cap may exceed it


@pytest.mark.parametrize("key_bits", T.KEY_BITS)
def test_c_keys_of_the_stand_alone_sorts(key_bits):
    for count in T.COUNTS:
        for shared in (False, True):
            for bounded in (False, True):
                keys, lo, hi = T.primitive_keys(key_bits, count, shared, bounded)
                assert len(keys) == count and keys.dtype == np.uint64
                assert key_bits == 64 or int(keys.max()) >> key_bits == 0
                if bounded:
                    assert lo <= int(keys.min()) and int(keys.max()) < hi
                    tops = np.unique(keys >> np.uint64(key_bits - min(key_bits, 8)))
                    assert len(tops) == (1 if shared and key_bits > 8 else min(3, 1 << min(key_bits, 8)))
                else:
                    assert (lo, hi) == (0, 0)
                if shared and key_bits > 8:
                    assert len(np.unique(keys >> np.uint64(min(8, key_bits - 8)))) == 1
                    assert len(np.unique(keys)) > min(100, 1 << (min(8, key_bits - 8) - 1))


def test_h_hashes():
    want = T.expected_hashes((12, 13), [0, 4096], lambda k: np.arange(k, dtype=np.uint64), "b" * 64)
    assert set(want) == {"keys-12", "keys-13", "bwt-12-0", "bwt-13-0", "bwt-12-4096", "bwt-13-4096"}
    T.check_hashes(want, dict(want))
    _fails(T.check_hashes, want, dict(want, **{"bwt-13-4096": "c" * 64}))
    _fails(T.check_hashes, want, dict(want, **{"keys-12": T.sha(np.arange(13, dtype=np.uint64))}))
    _fails(T.check_hashes, want, {key: v for key, v in want.items() if key != "bwt-12-0"})       # a child that stopped early
