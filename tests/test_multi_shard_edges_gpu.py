"""debwt_multi_build on the collections that break one-GPU paths (tests/shard_cases.py): all shards of a build on GPU 0 from
one process, 2, 3 and 8 of them.  Shards without keys, text slices without positions, shards of a handful of keys, blocks of
every size class behind a block base (qbase > 0) and a row base (Mbase, s0 > 0), separators on the slice boundaries, inputs
outside the reference's domain -- in both key modes, in one key range per shard and in several, and every shard's report
against the plan that tests/test_shard_cases_ref.py proves on the CPU.

Edges, the case that reaches them and the line of debwt_multi_get_shard_report that shows it (MI355X):
  shard without keys      homopolymer_only_one_record-k32, G = 2    shard 1: bins=[2731, 4096] keys=0 rows=6 blocks=0
                          (its 6 rows: the special suffixes G^0..G^5 '#', which sort behind every node of the other shard)
  ... and without bins    one_symbol_per_record-k32, G = 8          shard 6: bins=[4096, 4096] keys=0 rows=0 blocks=0
                          fewer_keys_than_shards-k32, G = 8         shard 0: bins=[0, 0] keys=0 rows=0
  slice without positions sp_code_shorter_than_32_symbols-k32, G = 8: slices 7 x (0, 0), (0, 61);
                                                                    shard 0: keys=3 keys_in=24 B, shard 7: keys_out=208 B
  shards of 1..6 keys     identical_records_of_34_bases...-k32, G = 8: keys = 2, 6, 0, 4, 4, 1, 5, 1
  large / medium / small block behind a block base
                          blocks_first_middle_last, G = 8, cap 6889 shard 7: key_ranges=6 blocks=144 large_blocks=1 max_block=2300
                                                                    (shard 0: max_block=2600; 700, 679, 642 rows in shards 3, 5, 1; 165..188 in the others)
                          deep_ties, G = 3, tune 1024               shard 2: blocks=13 large_blocks=1 max_block=4200
                          periodic, G = 8                           shard 6: large_blocks=1 max_block=56684; shard 7: bins=[4096, 4096]
  separators on slice boundaries   slice_edges_g*_*: p0 - 1, p0, p0 + 1, p0 + 5 (tests/test_shard_cases_ref.py)
  key ranges inside shards         every case twice: one range per shard, then the cap of Plan.range_cap (reads_20000, G = 8: 6 each)
  tune 32 / 1024 / 8192            blocks_first_middle_last and deep_ties at G = 3; periodic at G = 3
  reuse                            test_one_object_through_a_large_build_tiny_builds_with_empty_shards_and_back
A shard's context counts its OWN blocks and blue rows (blue_bound_num, blue_capacity), so the sums are compared with the
reference's or the oracle's totals and every shard's with the plan."""
import pytest

import shard_cases as SC
from shard_cases import CASES, plan_case

pytestmark = pytest.mark.gpu

STEPS_EVERY_SHARD_TAKES = {"shard_histogram", "shard_plan", "shard_classify_local", "shard_facts_export", "shard_classify_global",
                           "shard_sp_flags", "shard_sp_emit", "shard_sp_import", "shard_blue_route", "shard_blue_place", "blue_sort",
                           "bwt_assemble", "shard_export"}
STEPS_OF_MODE = {"rescan": {"kmer_sort_rle"}, "exchange": {"shard_partition_keys", "shard_sort_range", "shard_sort_end"}}


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def _set_cap(api, m, G, cap):
    for r in range(G):
        assert api._lib.lib().debwt_set_range_cap(m._shard_ctx(r), cap) == 0


def _counters(name, oracle):
    """(red_capacity, sp_len, special_branch_num, blue_bound_num, blue_capacity) of the whole collection, or None outside the
    reference's domain."""
    c = CASES[name]
    if c.expect == "golden":
        g = c.entry["counters"]
        return g["redCapacity"], g["spCodeLen"] - 32, g["specialBranchNum"], g["blueBoundNum"], g["blueCapacity"]
    if c.expect == "oracle":
        st = SC.oracle_stats(name, oracle)
        return st["red_capacity"], st["sp_len"], st["special_branch_num"], st["blue_bound_num"], st["blue_capacity"]
    return None


def _build_and_check(m, name, G, oracle, mode, ranges):
    """One build of the loaded case in key mode `mode`: result, device inverse walk, every shard's report.  ranges: per shard
    the number of key ranges the plan gives under the cap in force."""
    c, p = CASES[name], plan_case(name, G)
    tag = (name, G, mode, max(ranges))
    m.set_key_mode(mode)
    m.build()
    words, hrows, drow = m.fetch()
    diff = SC.check_result(name, oracle, words, hrows, drow)
    assert diff is None, tag + (diff,)
    assert m.verify_device()["ok"] == 1, tag
    reps = [m.shard_report(r) for r in range(G)]
    ms, s0 = m.stats()
    assert ms["ngpus"] == G and ms["rounds"] == max(ranges) and ms["key_mode"] == {"exchange": 0, "rescan": 1}[mode], tag
    # what every shard owns, against the definition
    assert [r["bins"] for r in reps] == [[p.bins[s], p.bins[s + 1]] for s in range(G)], tag
    assert [r["keys"] for r in reps] == p.keys, tag
    assert [r["rows"] for r in reps] == p.rows, tag
    assert [r["key_ranges"] for r in reps] == ranges, tag
    assert [r["blocks"] for r in reps] == [len(b) for b in p.blocks], tag
    assert [r["blue_rows"] for r in reps] == [int(b.sum()) for b in p.blocks], tag
    assert sum(r["rows"] for r in reps) == c.n and sum(r["keys"] for r in reps) == c.n - len(c.records()) * (c.k - 1), tag
    # the counters of a shard's context: its own blocks and blue rows; the red table and the SP code are the whole text's on
    # every shard -- the reference's counters (goldens), the oracle's (crafted collections)
    want = _counters(name, oracle)
    for r in reps:
        st = r["ctx"]
        assert (st["blue_bound_num"], st["blue_capacity"]) == (r["blocks"], r["blue_rows"]), tag + (r["shard"],)
        if want:
            assert (st["red_capacity"], st["sp_len"], st["special_branch_num"]) == want[:3], tag + (r["shard"],)
    if want:
        assert (sum(r["blocks"] for r in reps), sum(r["blue_rows"] for r in reps)) == want[3:], tag
    # what the shards sent is what the shards received
    for x in ("keys", "facts", "sp", "blue"):
        assert sum(r["bytes_in"][x] for r in reps) == sum(r["bytes_out"][x] for r in reps), tag + (x,)
    if mode == "rescan":
        assert all(r["bytes_in"]["keys"] == 0 and r["bytes_out"]["keys"] == 0 for r in reps), tag
    else:
        # the keys a shard owns and did not find in its own slice came in: all of them where its slice is empty
        for s, r in enumerate(reps):
            assert r["bytes_in"]["keys"] <= 8 * p.keys[s], tag
            if p.slices[s][0] == p.slices[s][1]:
                assert r["bytes_in"]["keys"] == 8 * p.keys[s] and r["bytes_out"]["keys"] == 0, tag + (s,)
    assert all(r["bytes_in"]["rows"] == 0 for r in reps[1:]), tag
    must = STEPS_EVERY_SHARD_TAKES | STEPS_OF_MODE[mode]
    for s, r in enumerate(reps):
        assert must <= set(r["ms"]), tag + (s, sorted(must - set(r["ms"])))     # also a shard without keys or positions
        assert r["ctx"]["n"] == c.n, tag
        if p.keys[s] == 0:
            # no node is the shard's: no block, no blue row, and no row but those of the special suffixes that sort into its bins
            assert r["blocks"] == 0 and r["blue_rows"] == 0 and r["rows"] == p.special[s], tag + (s,)
    for s in ([0] if c.large_first else []) + ([G - 1] if c.large_last else []):
        assert reps[s]["ctx"]["blue_large_blocks"] >= 1 and reps[s]["ctx"]["blue_max_block"] == int(p.blocks[s].max()), tag + (s,)
    return reps


def _run_case(api, oracle, name, G, tune):
    c, p = CASES[name], plan_case(name, G)
    cap, _ = p.range_cap()
    m = api.MultiDeBWT([0] * G, k=c.k, tune=tune)
    try:
        m.load_records(c.records())
        for cap_now in (None, cap):                                  # one key range per shard, then several where the text allows
            if cap_now:
                _set_cap(api, m, G, cap_now)
            ranges = [len(b) - 1 for b in p.ranges(cap_now)] if cap_now else [1] * G
            for mode in ("exchange", "rescan"):
                _build_and_check(m, name, G, oracle, mode, ranges)
    finally:
        m.close()


TUNES = ([(nm, 3, t) for nm in SC.BLOCK_CASES for t in (32, 1024)]      # cursor atomics behind a block base; the network alone
         + [("periodic", 3, 8192)])                                     # window rounds only
ALL = [(nm, G, 0) for nm, G in SC.case_worlds(SC.OUTSIDE + [SC.FEWER_KEYS] + SC.SMALL_GOLDENS + SC.MIDSIZE_GOLDENS + SC.BLOCK_CASES + ["periodic"] + SC.SLICE_EDGES)]


@pytest.mark.parametrize("name,G,tune", ALL + TUNES, ids=lambda v: str(v))
def test_shards_build_the_expected_bwt_and_report_what_the_plan_gives(api, oracle, name, G, tune):
    _run_case(api, oracle, name, G, tune)


def test_one_object_through_a_large_build_tiny_builds_with_empty_shards_and_back(api, oracle):
    """Eight shards, one object: the collection with blocks above the LDS capacity in several key ranges per shard, then one
    homopolymer record (seven shards without keys), then 61 symbols (seven slices without positions, shards of 3 and 4
    keys), then the first again -- neither the buffers nor the range fields of a build may show in the next."""
    G = 8
    m = api.MultiDeBWT([0] * G, k=32)
    try:
        cap, _ = plan_case("blocks_first_middle_last", G).range_cap()
        _set_cap(api, m, G, cap)
        for name in ("blocks_first_middle_last", "homopolymer_only_one_record-k32", "sp_code_shorter_than_32_symbols-k32",
                     "blocks_first_middle_last"):
            m.load_records(CASES[name].records())
            ranges = [len(b) - 1 for b in plan_case(name, G).ranges(cap)]
            for mode in ("exchange", "rescan"):
                _build_and_check(m, name, G, oracle, mode, ranges)
    finally:
        m.close()
