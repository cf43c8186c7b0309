"""The string graph over both strands on the GPU (debwt_fm_string_graph_both; FMIndex.string_graph_both) against its two
oracles: string_graph_ref.Graph on the doubled collection, and the strand-0 graph of an index built from the doubled
collection, byte for byte.  Stranded synthetic reads with crafted corners, min_overlap 1, tilings, wave and list
boundaries, batches cut by tiny limits, an index from files, sample steps, the capacity protocol, statistics, sequences."""
import ctypes

import numpy as np
import pytest

from bigraph_ref import crafted, doubled, sequences_both, stranded, unitigs_both
from overlap_ref import codes, rand_dna, revcomp, synthetic_reads
from string_graph_ref import Graph, flat, repeat_reads, sampled_reads, tiling
from test_fm_search_gpu import index_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


@pytest.fixture(scope="module")
def main(api):
    """(reads, names of the crafted ones, their index, the index of the doubled reads, reference graphs by min_overlap):
    built once, never changed"""
    strs, names = crafted(stranded(synthetic_reads(), 7))
    fm = index_of(api, codes(strs), s=8)
    fmd = index_of(api, codes(doubled(strs)), s=8)
    yield strs, names, fm, fmd, {L: Graph(doubled(strs), L) for L in (20, 41)}
    fm.close()
    fmd.close()


def check(res, G, lists):
    offs, edges = flat(lists)
    assert res.state.tolist() == G.state
    assert res.offsets.tolist() == offs
    assert [tuple(int(x) for x in e) for e in res.edges.tolist()] == edges
    assert len(res) == len(G.state) and [tuple(e) for e in res.out(len(G.state) - 1).tolist()] == lists[-1]


def same_bytes(a, b):
    assert a.state.tobytes() == b.state.tobytes() and a.offsets.tobytes() == b.offsets.tobytes()
    assert a.edges.tobytes() == b.edges.tobytes()


def graph_of(api, strs, min_overlap, s=8):
    """both lists of `strs` against the reference; the reference, the reduced result, the statistics of the reduced call and
    the unitig sequences (compared with the reference's here, while the index is open)"""
    fm = index_of(api, codes(strs), s=s)
    G = Graph(doubled(strs), min_overlap)
    try:
        red = fm.string_graph_both(min_overlap=min_overlap)
        check(red, G, G.I)
        st = fm.graph_both_stats()
        check(fm.string_graph_both(min_overlap=min_overlap, reduce=False), G, G.E)
        paths, circ = unitigs_both(G.state, G.I)
        seqs = red.sequences()
        assert seqs == sequences_both(strs, G.I, paths, circ)
    finally:
        fm.close()
    return G, red, st, seqs


@pytest.mark.parametrize("min_overlap", [20, 41])
def test_against_both_oracles(api, main, min_overlap):
    strs, names, fm, fmd, graphs = main
    G = graphs[min_overlap]
    for reduce, lists in ((True, G.I), (False, G.E)):
        res = fm.string_graph_both(min_overlap=min_overlap, reduce=reduce)
        check(res, G, lists)
        same_bytes(res, fmd.string_graph(min_overlap=min_overlap, reduce=reduce))
        assert res.reduced == reduce
    if min_overlap == 20:
        a, b, m = names["tail_a"], names["tail_b"], names["own_mirror"]
        everything = fm.string_graph_both(min_overlap=20, reduce=False)
        assert (2 * b + 1, 20) in [tuple(e) for e in everything.out(2 * a).tolist()]
        assert (2 * m + 1, 24) in [tuple(e) for e in everything.out(2 * m).tolist()]


def test_min_overlap_one(api, main):
    """a one-base seed occurs in a quarter of the text; edges from a read to its own mirror appear"""
    strs = main[0][:120]
    G, red, st, _ = graph_of(api, strs, 1)
    assert any(v == u ^ 1 for u, l in enumerate(G.E) for v, _ in l)
    assert st["seed_rows"] > 100 * st["seeds"] and max(len(l) for l in G.E) > 64


def test_tilings(api):
    g, reads = tiling(1, 2000, 60, 5)
    G, res, _, seqs = graph_of(api, stranded(reads, 3), 30)
    assert seqs in ([g], [revcomp(g)])
    g, reads = tiling(2, 1500, 60, 5, circle=True)
    G, res, _, seqs = graph_of(api, stranded(reads, 4), 30)
    assert res.unitigs()[2].tolist() == [1] and [len(s) for s in seqs] == [1500]


def test_repeat_and_mixed_lengths(api):
    G, res, _, _ = graph_of(api, stranded(repeat_reads()[1], 5), 30)
    assert len(res.unitigs()[2]) > 1
    G, _, st, _ = graph_of(api, stranded(sampled_reads(n=400), 6), 30)
    assert st["contained"] > 50 and st["reducible"] > st["kept"]


@pytest.mark.parametrize("nrec", [63, 64, 65])
def test_record_counts_at_a_wave(api, main, nrec):
    strs = main[0]
    graph_of(api, strs[len(strs) - nrec:], 20)                 # the crafted reads and the reads before them


def seed_copies(counts=(0, 1, 63, 64, 65, 300), seed=13):
    """per count c a read that ends in a flank T of 20 b and c reads that hold rc T at base 30: every third one goes on as
    a true tail-to-tail overlap of 20, 22 or 24 bases, the others with bases that do not fit or run past the read"""
    rng = np.random.default_rng(seed)
    out = []
    for c in counts:
        src = rand_dna(rng, 50)
        out.append(src)
        for k in range(c):
            if k % 3 == 0:
                out.append(rand_dna(rng, 30) + revcomp(src[-(20 + 2 * (k // 3 % 3)):]))
            elif k % 3 == 1:
                out.append(rand_dna(rng, 30) + revcomp(src[-20:]) + rand_dna(rng, 8))
            else:
                out.append(rand_dna(rng, 30) + revcomp(src[-20:]) + rand_dna(rng, 45))
    return [out[int(i)] for i in rng.permutation(len(out))]


def test_seed_occurrences_at_a_wave(api):
    strs = seed_copies()
    G, _, st, _ = graph_of(api, strs, 20)
    assert st["seed_rows"] >= 1 + 63 + 64 + 65 + 300 and 100 < st["tail_hits"] < st["seed_rows"]
    assert st["edges_kind"][1] >= 100


def test_lists_beyond_a_wave(api):
    """70 reads end in a common 25 b, 70 start with it or with its last 20: out-lists of 140 entries at two lengths"""
    rng = np.random.default_rng(17)
    c = rand_dna(rng, 25)
    strs = [rand_dna(rng, 40) + c for _ in range(70)] + [c + rand_dna(rng, 40) for _ in range(70)]
    strs += [c[5:] + rand_dna(rng, 40) for _ in range(70)]
    G, _, _, _ = graph_of(api, stranded(strs, 8), 20)
    assert max(len(l) for l in G.E) == 140 and {len(l) for l in G.E[0::2]} >= {0, 140} and {len(l) for l in G.E[1::2]} >= {0, 140}


def test_batches_do_not_change_results(api, main, monkeypatch):
    strs, _, fm, _, graphs = main
    G = graphs[20]
    fm.string_graph_both(min_overlap=20)
    base = fm.graph_both_stats()["launches"]
    for slots, hits in (("64", None), (None, "64"), ("64", "64")):
        for name, v in (("DEBWT_FM_OVERLAP_SLOTS", slots), ("DEBWT_FM_OVERLAP_HITS", hits)):
            monkeypatch.setenv(name, v) if v else monkeypatch.delenv(name, raising=False)
        check(fm.string_graph_both(min_overlap=20), G, G.I)
        assert fm.graph_both_stats()["launches"] > base + 20   # many batches, or many chunks of one batch
        check(fm.string_graph_both(min_overlap=20, reduce=False), G, G.E)


# Every field of graph_both_stats() that is no time, on the crafted set at min_overlap 20, by (limits, reduce).  Recorded on
# an MI355X at the commit before the two graph builders shared one batch loop: they are sums and counts, and the batches
# depend on the input and the two limits alone.  A difference means a launch, a batch or a buffer changed.
_COUNTS = {"records": 449, "kept": 385, "duplicates": 10, "contained": 54, "hits": 3587, "edges": 5845, "edge_bytes": 46760,
           "selfrc": 1, "seeds": 385, "seed_rows": 1498, "tail_hits": 1419, "edges_kind": [1500, 1419, 1426, 1500]}
PINNED = {
    (None, True): dict(_COUNTS, reducible=5098, lookups=5098, launches=18, scratch_bytes=1064397),
    (None, False): dict(_COUNTS, reducible=0, lookups=0, launches=15, scratch_bytes=1064397),
    ("64", True): dict(_COUNTS, reducible=5098, lookups=5098, launches=4211, scratch_bytes=13423),
    ("64", False): dict(_COUNTS, reducible=0, lookups=0, launches=4208, scratch_bytes=13423),
}


@pytest.mark.parametrize("limits", [None, "64"])
def test_stats_are_pinned(api, main, monkeypatch, limits):
    fm = main[2]
    for name in ("DEBWT_FM_OVERLAP_SLOTS", "DEBWT_FM_OVERLAP_HITS"):
        monkeypatch.setenv(name, limits) if limits else monkeypatch.delenv(name, raising=False)
    got = {}
    for reduce in (True, False):
        fm.string_graph_both(min_overlap=20, reduce=reduce)
        got[limits, reduce] = {k: v for k, v in fm.graph_both_stats().items() if not k.startswith("ms_")}
        print("PINNED[%r, %r] = %r" % (limits, reduce, got[limits, reduce]))
    assert got == {k: v for k, v in PINNED.items() if k[0] == limits}


def test_index_from_files_and_sample_steps(api, main):
    strs, _, own, _, graphs = main
    G = graphs[20]
    d = api.DeBWT(k=32)
    d.load_records(codes(strs))
    d.build()
    words, hrows, drow = d.fetch()
    d.close()
    for s in (4, 32):
        fm = index_of(api, codes(strs), s=s)
        check(fm.string_graph_both(min_overlap=20), G, G.I)
        if s == 4:                                             # opened from rows and samples alone: the call restores the text
            opened = api.FMIndex.open(words, sum(len(x) + 1 for x in strs), hrows, drow, fm.samples(), sa_sample=4)
            check(opened.string_graph_both(min_overlap=20), G, G.I)
            assert opened.extract_stats()["bases"] == opened.n
            check(opened.string_graph_both(min_overlap=20, reduce=False), G, G.E)
            opened.close()
        fm.close()


def raw_call(fm, min_overlap, flags, capacity):
    from debwt_amd import _lib
    nn = 2 * fm.nrec
    state = np.full(nn, 9, dtype=np.uint8)
    offs = np.full(nn + 1, 77, dtype=np.uint64)
    edges = np.zeros(max(capacity, 1), dtype=np.dtype([("record", np.uint32), ("length", np.uint32)]))
    rc = fm._L.debwt_fm_string_graph_both(fm._h, min_overlap, flags, state.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                          offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                          edges.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmEdge)) if capacity else None, capacity)
    return rc, state, offs, edges[:capacity]


def test_errors_and_capacity(api, main):
    strs, _, fm, _, graphs = main
    G = graphs[20]
    offs, edges = flat(G.I)
    for cap in (0, len(edges) - 1):
        rc, state, o, _ = raw_call(fm, 20, 0, cap)
        assert rc == -5 and state.tolist() == G.state and o.tolist() == offs
        assert str(len(edges)) in fm._L.debwt_fm_last_error(fm._h).decode()
    rc, state, o, e = raw_call(fm, 20, 0, len(edges))
    assert rc == 0 and o.tolist() == offs and [tuple(x) for x in e.tolist()] == edges
    rc, _, o, e = raw_call(fm, 20, 1, sum(len(l) for l in G.E))
    assert rc == 0 and [tuple(x) for x in e.tolist()] == flat(G.E)[1]
    assert raw_call(fm, 0, 0, 100)[0] == -1 and "min_overlap" in fm._L.debwt_fm_last_error(fm._h).decode()
    assert raw_call(fm, 20, 2, 100)[0] == -1 and "flags" in fm._L.debwt_fm_last_error(fm._h).decode()
    with pytest.raises(api.DebwtError):
        fm.string_graph_both(min_overlap=0)
    far = fm.string_graph_both(min_overlap=500)                # longer than every record: states, no edges
    assert far.state.tolist() == G.state and len(far.edges) == 0 and not far.offsets.any()


def test_strand_zero_graph_is_unchanged(api, main):
    strs, _, fm, _, _ = main
    F = Graph(strs, 20)
    before = fm.string_graph(min_overlap=20)
    st0 = fm.graph_stats()
    fm.string_graph_both(min_overlap=20)
    assert {k: v for k, v in fm.graph_stats().items() if not k.startswith("ms_")} == {k: v for k, v in st0.items() if not k.startswith("ms_")}
    after = fm.string_graph(min_overlap=20)
    same_bytes(before, after)
    assert before.state.tolist() == F.state and [tuple(int(x) for x in e) for e in before.edges.tolist()] == flat(F.I)[1]


def test_stats_add_up(api, main):
    strs, _, fm, _, graphs = main
    G = graphs[20]
    res = fm.string_graph_both(min_overlap=20)
    st = fm.graph_both_stats()
    ne, nr = sum(len(l) for l in G.E), sum(sum(r) for r in G.red)
    kinds = [0, 0, 0, 0]
    for u, l in enumerate(G.E):
        for v, _ in l:
            kinds[2 * (u & 1) + (v & 1)] += 1
    assert st["edges"] == ne == sum(st["edges_kind"]) and st["edges_kind"] == kinds
    assert st["reducible"] == nr and ne - nr == len(res.edges) and st["edge_bytes"] == 8 * ne
    assert st["records"] == len(strs) == st["kept"] + st["duplicates"] + st["contained"]
    reads = G.state[0::2]
    assert (st["kept"], st["duplicates"], st["contained"]) == (reads.count(0), reads.count(1), reads.count(2))
    assert st["selfrc"] == 1 and st["seeds"] == st["kept"] and st["tail_hits"] <= st["seed_rows"] and st["tail_hits"] >= kinds[1]
    assert st["hits"] >= kinds[0] + kinds[2] and st["lookups"] >= st["reducible"] and st["launches"] >= 12
    assert min(st[k] for k in ("ms_walk", "ms_build", "ms_tail", "ms_merge", "ms_reduce", "ms_wall")) > 0
    # without a self-rc read every ++ edge has a -- mirror; +- and -+ edges mirror onto their own kind
    base = stranded(synthetic_reads(), 7)
    _, _, st, _ = graph_of(api, base, 20)
    k = st["edges_kind"]
    assert st["selfrc"] == 0 and k[0] == k[3] and min(k) > 1000 and st["edges"] == sum(k)
