"""CPU: the collections of tests/shard_cases.py reach the edges the sharded GPU tests (test_multi_shard_edges_gpu.py,
test_sharded_edges_gpu.py) are there for -- proven from plan() alone, the numpy restatement of the splitter, slice and
range rules, independent of the code under test -- and their expected results are sound: the oracle's build equals the
BWT by definition on the crafted collections (the host inverse walk where the naive sort would take too long)."""
import numpy as np
import pytest

import shard_cases as SC
from shard_cases import CASES, WORLDS, plan_case

# owned keys per shard, by the C host's splitter rule over the census of the node keys
OWNED_KEYS = {
    ("homopolymer_only_one_record-k32", 501): ([470, 0], [470, 0, 0], [470, 0, 0, 0, 0, 0, 0, 0]),
    ("tandem_repeat_of_two_symbols-k32", 382): ([160, 160], [160, 160, 0], [160, 0, 0, 0, 160, 0, 0, 0]),
    ("one_symbol_per_record-k32", 274): ([100, 50], [100, 0, 50], [100, 0, 0, 0, 0, 50, 0, 0]),
    ("one_symbol_per_record-k12", 274): ([140, 90], [140, 23, 67], [140, 0, 0, 0, 23, 67, 0, 0]),
    ("identical_records_of_34_bases_and_a_prefix_of_them-k32", 147): ([12, 11], [8, 8, 7], [2, 6, 0, 4, 4, 1, 5, 1]),
    ("sp_code_shorter_than_32_symbols-k32", 61): ([15, 15], [10, 10, 10], [3, 4, 4, 4, 3, 4, 4, 4]),
}


@pytest.mark.parametrize("name,n", sorted(OWNED_KEYS))
def test_small_collections_leave_shards_without_keys_or_with_a_handful(name, n):
    assert CASES[name].n == n
    for G, want in zip(WORLDS, OWNED_KEYS[(name, n)]):
        assert plan_case(name, G).keys == want, (name, G)


def test_every_plan_tiles_key_space_and_text():
    for name, c in CASES.items():
        for G in c.worlds:
            p = plan_case(name, G)
            assert p.bins[0] == 0 and p.bins[-1] == SC.SHARD_BINS and all(a <= b for a, b in zip(p.bins, p.bins[1:]))
            assert sum(p.keys) == p.n - p.nrec * (c.k - 1) == int(p.hist.sum()), (name, G)
            assert p.slices[0][0] == 0 and p.slices[-1][1] == p.n
            assert all(a[1] == b[0] and a[0] % 32 == 0 for a, b in zip(p.slices, p.slices[1:])) and p.slices[-1][0] % 32 == 0


def test_texts_below_32_symbols_per_rank_have_empty_slices():
    seen = set()
    for name, c in CASES.items():
        for G in c.worlds:
            p = plan_case(name, G)
            if p.n < 32 * G:
                assert all(p0 == p1 == 0 for p0, p1 in p.slices[:-1]) and p.slices[-1] == (0, p.n), (name, G)
                seen.add((p.n, G))
            else:
                assert all(p1 > p0 for p0, p1 in p.slices), (name, G)
    # n = 61 at every G; the collections of 123, 147 and 193 symbols at G = 8: the last rank scans the whole text alone
    assert seen == {(61, 2), (61, 3), (61, 8), (123, 8), (147, 8), (193, 8), (34, 8)}


def test_shards_that_start_behind_the_last_bin_or_end_at_the_first():
    """A shard whose splitter target lies inside bin 4095 owns the bins [4096, 4096): at k = 32 their first key would be
    2^64.  More shards than keys: shards of the bins [0, 0)."""
    hit = {(nm, G) for nm, c in CASES.items() for G in c.worlds if c.k == 32 and SC.SHARD_BINS in plan_case(nm, G).bins[:G]}
    assert {("one_symbol_per_record-k32", 8), ("periodic", 8)} <= hit
    p = plan_case("one_symbol_per_record-k32", 8)
    assert p.bins[6:] == [4096, 4096, 4096] and p.keys[5] == 50 and p.special[6:] == [0, 0]
    p = plan_case(SC.FEWER_KEYS, 8)
    assert sum(p.keys) == 3 and p.bins[:3] == [0, 0, 0] and p.keys[:2] == [0, 0] and p.special[:2] == [0, 0]
    assert p.n == 34 and all(s == (0, 0) for s in p.slices[:7])


def _in(sizes, lo, hi):
    return int(((sizes >= lo) & (sizes <= hi)).sum())


def test_blocks_first_middle_last_puts_every_block_class_behind_a_block_base():
    """A block above 2048 rows in the first and in the last shard, a block of 257..2048 rows in a middle shard, blocks of
    65..256 rows in every one of 8 shards -- also when only nodes with two distinct predecessors count."""
    for G in WORLDS:
        p = plan_case("blocks_first_middle_last", G)
        for sizes in (p.blocks, p.strict):
            assert sizes[0].max() > 2048 and sizes[G - 1].max() > 2048, G
            if G > 2:
                assert any(_in(sizes[s], 257, 2048) for s in range(1, G - 1)), G
        assert [int(b.max()) for b in p.blocks] == [int(b.max()) for b in p.strict]
    p = plan_case("blocks_first_middle_last", 8)
    assert all(_in(p.strict[s], 65, 256) >= 1 for s in range(8))
    assert int(plan_case("blocks_first_middle_last", 3).blocks[1].max()) == 700
    assert [int(plan_case("blocks_first_middle_last", G).blocks[G - 1].max()) for G in WORLDS] == [2300] * 3
    assert [int(plan_case("blocks_first_middle_last", G).blocks[0].max()) for G in WORLDS] == [2600] * 3


def test_deep_ties_puts_its_large_block_into_the_last_shard():
    for G in WORLDS:
        p = plan_case("deep_ties", G)
        assert int(p.strict[G - 1].max()) == int(p.blocks[G - 1].max()) == 4200, G


def test_periodic_has_large_blocks_in_shards_behind_the_first_and_an_empty_shard_of_eight():
    for G in WORLDS:
        p = plan_case("periodic", G)
        assert sum(int(b.max()) > 2048 for b in p.blocks[1:] if len(b)) >= 1, G
    assert plan_case("periodic", 8).keys[7] == 0          # one bin (a run of T) holds more than an eighth of all keys


def test_case_flags_say_what_the_plan_says():
    for name, c in CASES.items():
        for G in c.worlds:
            p = plan_case(name, G)
            if c.large_first:
                assert p.blocks[0].max() > 2048, (name, G)
            if c.large_last:
                assert p.blocks[G - 1].max() > 2048, (name, G)


@pytest.mark.parametrize("name", [nm for nm in SC.SLICE_EDGES if nm.endswith("-k32")])
def test_slice_edges_put_separators_on_the_slice_boundaries(name, oracle):
    c = CASES[name]
    (G,) = c.worlds
    recs = c.records()
    assert 6 <= len(recs) <= 12 and all(33 <= len(r) <= 400 for r in recs)
    p = plan_case(name, G)
    seps = set((np.cumsum([len(r) + 1 for r in recs]) - 1).tolist())
    for rank, kind in c.edges.items():
        p0 = p.slices[rank][0]
        assert p0 > 0
        near = sorted(s - p0 for s in seps if abs(s - p0) <= 31)
        if kind == "sep_at_p0_minus_1":
            assert near == [-1]                                     # the slice starts with the first base of a record
        elif kind == "sep_at_p0":
            assert near == [0]                                      # ... with a separator
        elif kind == "sep_at_p0_plus_1":
            assert near == [1]                                      # ... with the last base of a record
        else:
            assert near == [5]                                      # the k - 1 positions before the separator straddle p0
            for k in (12, 32):
                assert p0 + 5 - (k - 1) < p0 < p0 + 5
    # every kind occurs over the variants of this G
    kinds = set()
    for nm in SC.SLICE_EDGES:
        if CASES[nm].worlds == (G,):
            kinds |= set(CASES[nm].edges.values())
    assert kinds == set(SC.SLICE_EDGE_KINDS)
    for k in (12, 32):
        st = oracle.build_bwt(oracle.sym_from_codes(recs), k)[3]
        assert st["special_branch_num"] > 0 and st["blue_bound_num"] > 0, (name, k)


def test_python_host_splitters_equal_the_c_hosts_and_leave_empty_shards():
    from debwt_amd.sharded import plan_splitters
    for name, c in CASES.items():
        for G in c.worlds:
            p = plan_case(name, G)
            bins, _ = plan_splitters(p.hist.astype(np.uint64), G)
            assert bins == p.bins, (name, G)
    for world in (2, 3):
        hist = plan_case("homopolymer_only_one_record-k32", 2).hist
        bins, cum = plan_splitters(hist.astype(np.uint64), world)
        sizes = [int(cum[bins[r + 1]] - cum[bins[r]]) for r in range(world)]
        assert min(sizes) == 0 and sum(sizes) == 470, (world, sizes)


def test_range_caps_cut_the_fullest_shard_into_3_to_40_ranges_where_the_interface_allows():
    """debwt_set_range_cap takes 4096 instances or more, so only a shard of more than two such ranges can be cut into three:
    every collection above a few 10^4 symbols is; below, the cap is 4096 and the plan says how many ranges that makes."""
    for name, c in CASES.items():
        for G in c.worlds:
            p = plan_case(name, G)
            cap, nfull = p.range_cap()
            counts = [len(b) - 1 for b in p.ranges(cap)]
            assert cap >= SC.MIN_RANGE_CAP and max(counts) <= SC.MAX_RANGES and nfull == counts[int(np.argmax(p.keys))]
            if name in SC.BLOCK_CASES + SC.MIDSIZE_GOLDENS + ["periodic"]:
                assert 3 <= nfull <= 40, (name, G, cap, nfull)
            elif max(p.keys) <= 2 * SC.MIN_RANGE_CAP:
                assert cap == SC.MIN_RANGE_CAP and nfull <= 2, (name, G)


def test_case_list_and_sizes():
    assert len(SC.OUTSIDE) == 18 and len(SC.SMALL_GOLDENS) == 11 and sorted(SC.MIDSIZE_GOLDENS) == ["pan_4x20k-k12", "reads_20000-k32"]
    assert all(CASES[nm].entry["n"] == CASES[nm].n for nm in SC.SMALL_GOLDENS)
    assert CASES["blocks_first_middle_last"].n == 255_218
    for name, c in CASES.items():
        if name in SC.MIDSIZE_GOLDENS:
            assert c.entry["n"] <= 4_553_304
        elif name == "periodic":
            assert c.n == 334_700                       # the recipe of the parity suite, symbol for symbol
        else:
            assert c.n < 300_000, name


@pytest.mark.parametrize("name", ["blocks_first_middle_last", "deep_ties"] + [nm for nm in SC.SLICE_EDGES])
def test_expected_results_of_crafted_cases_equal_the_definition(name, oracle):
    c = CASES[name]
    sym = oracle.sym_from_codes(c.records())
    w, h, d = SC.expected(name, oracle)
    assert np.array_equal(oracle.unpack_bwt(w, len(sym), h, d), oracle.naive_bwt(sym))


def test_expected_result_of_periodic_inverts_to_the_text(oracle):
    """Runs of thousands of equal symbols are beyond the naive suffix sort: the host inverse walk over the oracle's rows
    must give back the text."""
    from debwt_amd import api
    sym = oracle.sym_from_codes(CASES["periodic"].records())
    w, h, d = SC.expected("periodic", oracle)
    rc, inv = api.verify_inverse(w, len(sym), h, d)
    assert rc == 0 and np.array_equal(inv, sym)


@pytest.mark.parametrize("name", ["blocks_first_middle_last", "deep_ties", "periodic", "slice_edges_g8_0-k12", "slice_edges_g3_1-k32"])
def test_blocks_of_the_plan_are_the_oracles(name, oracle):
    c = CASES[name]
    st = oracle.build_bwt(oracle.sym_from_codes(c.records()), c.k)[3]
    for G in c.worlds:
        p = plan_case(name, G)
        assert sum(len(b) for b in p.blocks) == st["blue_bound_num"] and sum(int(b.sum()) for b in p.blocks) == st["blue_capacity"], (name, G)
