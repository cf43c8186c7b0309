"""Pair counts of the radix sort: a pass whose next digit takes few values counts both digits in one read of the keys, and
the pass behind it takes its chunk histograms and its chunks from tables instead of a count pass of its own.
The sorted arrays and everything built from them stay bit-identical; DEBWT_HIST_EVERY_PASS=1 restores the count pass in
front of every pass."""
import functools

import numpy as np
import pytest

from conftest import golden_manifest, golden_records

pytestmark = pytest.mark.gpu

BASE = 37                      # smallest top byte of the drawn keys: the derived rows do not start at row 0


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def _derived_passes(api):
    return int(api._lib.lib().debwt_radix_pair_passes())


@functools.lru_cache(maxsize=None)
def _keys(count, nv):
    """(keys, sorted keys): the top byte takes the nv values BASE .. BASE + nv - 1 (all of them when count allows)."""
    rng = np.random.default_rng(1000 * nv + count % 997)
    top = rng.integers(0, nv, size=count, dtype=np.uint64)
    top[:nv] = np.arange(nv, dtype=np.uint64)
    keys = ((top + np.uint64(BASE)) << np.uint64(56)) | rng.integers(0, 1 << 56, size=count, dtype=np.uint64)
    keys.setflags(write=False)
    ref = np.sort(keys)
    ref.setflags(write=False)
    return keys, ref


def _sort(api, keys, algo, key_lo, key_hi):
    import torch
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    tmp = torch.empty_like(dk)
    d = api.DeBWT(k=32, sort_algo=algo)
    before = _derived_passes(api)
    d.radix_sort_device(dk.data_ptr(), tmp.data_ptr(), len(keys), 64, key_lo=key_lo, key_hi=key_hi)
    out = dk.cpu().numpy().view(np.uint64)
    d.close()
    return out, _derived_passes(api) - before


# algo 1 runs eight array passes at every count; the hybrid sort (3) runs two from 2^14 keys on, one below
@pytest.mark.parametrize("algo", [1, 3])
@pytest.mark.parametrize("count", [4097, 1 << 20, 3_000_001])
@pytest.mark.parametrize("nv", [1, 5, 40, 64, 65])
def test_sort_with_narrow_top_byte(api, nv, count, algo):
    keys, ref = _keys(count, nv)
    out, derived = _sort(api, keys, algo, BASE << 56, (BASE + nv) << 56)
    assert np.array_equal(out, ref)
    pairs = nv <= 64 and (algo == 1 or count >= (1 << 14))        # 65 values: 256 x 65 cells are more than 64 KB of LDS
    # (the hybrid sort adds derived passes of its own when buckets come out oversize -- a top byte of one value at any
    # count: the auxiliary passes over the gathered stretches pair up too)
    assert derived == int(pairs) if algo == 1 else derived >= int(pairs)


def test_sort_without_bounds_counts_every_pass(api):
    keys, ref = _keys(1 << 20, 5)
    out, derived = _sort(api, keys, 1, 0, 0)
    assert np.array_equal(out, ref) and derived == 0


def test_switch_restores_every_count_pass(api, monkeypatch):
    monkeypatch.setenv("DEBWT_HIST_EVERY_PASS", "1")
    keys, ref = _keys(1 << 20, 40)
    out, derived = _sort(api, keys, 1, BASE << 56, (BASE + 40) << 56)
    assert np.array_equal(out, ref) and derived == 0


@pytest.mark.parametrize("algo", [1, 3])
def test_keys_share_their_top_two_bytes(api, algo):
    """One value of the counted digit and one of the derived digit: every unit but one per chunk is empty."""
    n = 1 << 20
    rng = np.random.default_rng(5)
    keys = (np.uint64(0x2A5C) << np.uint64(48)) | rng.integers(0, 1 << 48, size=n, dtype=np.uint64)
    out, derived = _sort(api, keys, algo, 0x2A << 56, 0x2B << 56)
    assert np.array_equal(out, np.sort(keys)) and derived >= 1


@pytest.mark.parametrize("algo", [1, 3])
def test_one_unit_holds_a_whole_chunk(api, algo):
    """Input in ascending order: a chunk of the counted pass carries one or two values of its digit, so a unit is as long
    as a chunk of the derived pass (or nearly), and chunks come out empty or twice the target."""
    keys, ref = _keys(3_000_001, 40)
    out, derived = _sort(api, np.ascontiguousarray(ref), algo, BASE << 56, (BASE + 40) << 56)
    assert np.array_equal(out, ref) and derived >= 1
    # the second digit from the top constant over long stretches of the input, the top byte random inside them
    rng = np.random.default_rng(6)
    n = 1 << 20
    keys = ((rng.integers(0, 40, size=n, dtype=np.uint64) + np.uint64(BASE)) << np.uint64(56)) | \
           ((np.arange(n, dtype=np.uint64) >> np.uint64(15)) << np.uint64(48)) | rng.integers(0, 1 << 48, size=n, dtype=np.uint64)
    out, derived = _sort(api, keys, algo, BASE << 56, (BASE + 40) << 56)
    assert np.array_equal(out, np.sort(keys)) and derived >= 1


def test_keys_outside_the_bounds_are_refused(api):
    keys, _ = _keys(4097, 5)
    with pytest.raises(Exception):
        _sort(api, keys, 1, BASE << 56, (BASE + 4) << 56)


# ---- the build -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def collection(oracle):
    from debwt_amd import synth
    recs = synth.pan_genome(6_250_000, 4)                         # 25 Mbp
    ow, oh, od, ost = oracle.build_bwt(oracle.sym_from_codes(recs), 32)
    return recs, ow, oh, od


def _build(api, recs, cap):
    d = api.DeBWT(k=32)
    d.load_records(recs)
    d.set_range_cap(cap)
    before = _derived_passes(api)
    d.build()
    out = d.fetch()
    derived = _derived_passes(api) - before
    d.close()
    return out, derived


# 25 M node instances: five near-equal ranges of 5 M keys (three array passes behind the text pass: the last two pair up);
# a cap of M / 4.1 fills four ranges to 17/16 of a fifth and leaves a short last range of under 2^22 keys, which takes
# one array pass only and so the old path
@pytest.mark.parametrize("divide", [4.9, 4.1], ids=["five_even_ranges", "short_last_range"])
def test_build_in_key_ranges(api, collection, monkeypatch, divide):
    recs, ow, oh, od = collection
    m = sum(len(r) for r in recs)
    cap = int(m / divide)
    (words, hrows, drow), derived = _build(api, recs, cap)
    assert derived >= 4                                           # the key ranges above 2^22 keys took the pair form
    assert np.array_equal(words, ow) and np.array_equal(hrows, oh) and drow == od
    monkeypatch.setenv("DEBWT_HIST_EVERY_PASS", "1")
    (w2, h2, d2), derived = _build(api, recs, cap)
    assert derived == 0
    assert np.array_equal(words, w2) and np.array_equal(hrows, h2) and drow == d2


# ---- blue entries ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pan_6x60k", "ecoli_4.6M"])
def test_blue_entry_sort_pairs_its_passes(api, monkeypatch, name):
    """The routed blue entries are sorted by the bits of their block id, spread evenly over the passes: 498 blocks take
    passes of 5 + 4 bits, 11,146 blocks 7 + 7 (128 x 128 cells: the largest joint count there is); the second is derived."""
    entry = next(e for e in golden_manifest() if e["name"] == name and e["k"] == 32)
    assert entry["counters"]["blueCapacity"] > 1
    recs = golden_records(entry)

    def build():
        d = api.DeBWT(k=32)
        d.load_records(recs)
        before = _derived_passes(api)
        d.kmer_sort_rle()
        d.classify()
        d.sp_generate()
        blue = d.fetch_array(api.ARR_BLUE)                        # the entries as the sort left them
        d.blue_sort()
        d.bwt_assemble()
        out = d.fetch()
        d.close()
        return blue, out, _derived_passes(api) - before

    blue, (words, hrows, drow), derived = build()
    assert derived >= 1
    monkeypatch.setenv("DEBWT_HIST_EVERY_PASS", "1")
    blue2, (w2, h2, d2), derived = build()
    assert derived == 0
    assert np.array_equal(blue, blue2)
    assert np.array_equal(words, w2) and np.array_equal(hrows, h2) and drow == d2
