"""The string graph on the GPU (debwt_fm_string_graph, debwt_fm_edges_reduce; FMIndex.string_graph, api.edges_reduce)
against the definitions of string_graph_ref.py: states, offsets and the whole ordered edge list compared exactly, with
and without the reduction, on the synthetic read set, tilings of a line and of a circle, a repeat, reads of mixed lengths
and golden reads; an index from files, the capacity protocol, errors, batches cut by tiny limits, unitig sequences,
statistics; the reduction kernel alone on crafted lists and on a list with mismatches."""
import ctypes

import numpy as np
import pytest

from conftest import golden_outputs, golden_records
from overlap_mm_ref import mutated_reads
from overlap_ref import codes, synthetic_reads
from string_graph_ref import Graph, flat, reducible, repeat_reads, sampled_reads, tiling
from test_fm_index_gpu import text_of
from test_fm_search_gpu import entry_named, index_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


@pytest.fixture(scope="module")
def synth(api):
    """(record strings, their index, the reference graphs by min_overlap): built once, never changed"""
    strs = synthetic_reads()
    fm = index_of(api, codes(strs), s=4)
    yield strs, fm, {L: Graph(strs, L) for L in (1, 20, 41)}
    fm.close()


def rec_strings(recs):
    return ["".join("ACGT"[c] for c in np.asarray(r).tolist()) for r in recs]


def check(res, G, lists):
    offs, edges = flat(lists)
    assert res.state.tolist() == G.state
    assert res.offsets.tolist() == offs
    assert [tuple(int(x) for x in e) for e in res.edges.tolist()] == edges
    assert len(res) == len(G.state) and [tuple(e) for e in res.out(len(G.state) - 1).tolist()] == lists[-1]


def graph_of(api, strs, min_overlap, s=8):
    fm = index_of(api, codes(strs), s=s)
    G = Graph(strs, min_overlap)
    try:
        red = fm.string_graph(min_overlap=min_overlap)
        check(red, G, G.I)
        st = fm.graph_stats()
        check(fm.string_graph(min_overlap=min_overlap, reduce=False), G, G.E)
        assert red.sequences() == G.seqs
    finally:
        fm.close()
    return G, red, st


@pytest.mark.parametrize("min_overlap", [1, 20, 41])
def test_synthetic_read_set(api, synth, min_overlap):
    strs, fm, graphs = synth
    G = graphs[min_overlap]
    res = fm.string_graph(min_overlap=min_overlap)
    check(res, G, G.I)
    assert res.reduced
    st = fm.graph_stats()
    ne, nr = sum(len(l) for l in G.E), sum(sum(r) for r in G.red)
    assert st["records"] == len(strs) and st["kept"] + st["duplicates"] + st["contained"] == st["records"]
    assert (st["kept"], st["duplicates"], st["contained"]) == (G.state.count(0), G.state.count(1), G.state.count(2))
    assert st["edges"] == ne and st["reducible"] == nr and st["edges"] - st["reducible"] == len(res.edges)
    assert st["hits"] >= st["edges"] and st["lookups"] >= st["reducible"] and st["edge_bytes"] == 8 * ne
    assert st["launches"] >= 8 and st["scratch_bytes"] > 0
    assert st["ms_walk"] > 0 and st["ms_build"] > 0 and st["ms_reduce"] > 0 and st["ms_wall"] > 0
    everything = fm.string_graph(min_overlap=min_overlap, reduce=False)
    check(everything, G, G.E)
    st = fm.graph_stats()
    assert not everything.reduced and st["edges"] == ne == len(everything.edges) and st["reducible"] == 0 and st["ms_reduce"] == 0


def test_unitigs_and_sequences(api, synth):
    strs, fm, graphs = synth
    G = graphs[20]
    res = fm.string_graph(min_overlap=20)
    uoff, mem, circ = res.unitigs()
    assert [mem[int(uoff[u]):int(uoff[u + 1])].tolist() for u in range(len(circ))] == G.paths
    assert circ.tolist() == G.circular
    assert res.sequences() == G.seqs and max(len(s) for s in G.seqs) == 2999


def test_tiling_of_a_line(api):
    g, reads = tiling(1, 2000, 60, 5)
    G, res, _ = graph_of(api, reads, 30)
    assert G.seqs == [g]                                       # graph_of compared the GPU's sequences with these


def test_tiling_of_a_circle(api):
    g, reads = tiling(2, 1500, 60, 5, circle=True)
    G, res, _ = graph_of(api, reads, 30)
    assert res.unitigs()[2].tolist() == [1] and [len(s) for s in G.seqs] == [1500]


def test_repeat_gives_branches(api):
    G, res, _ = graph_of(api, repeat_reads()[1], 30)
    assert len(G.paths) > 1 and int((res.offsets[1:] - res.offsets[:-1]).max()) == 2


def test_reads_of_mixed_lengths(api):
    G, _, st = graph_of(api, sampled_reads(), 30)
    assert st["contained"] > 300 and st["duplicates"] > 0 and st["reducible"] > st["kept"]


def test_golden_reads(api):
    strs = rec_strings(golden_records(entry_named("reads_20000")))[:2000]
    G, _, st = graph_of(api, strs, 30)
    assert st["edges"] > 0 and st["records"] == 2000


def test_index_from_files(api, synth):
    """an index opened from rows and samples alone, no text given: the graph restores it"""
    strs, own, graphs = synth
    d = api.DeBWT(k=32)
    d.load_records(codes(strs))
    d.build()
    words, hrows, drow = d.fetch()
    d.close()
    opened = api.FMIndex.open(words, sum(len(s) + 1 for s in strs), hrows, drow, own.samples(), sa_sample=4)
    G = graphs[20]
    res = opened.string_graph(min_overlap=20)
    check(res, G, G.I)
    assert opened.extract_stats()["bases"] == opened.n         # the restore ran inside the call
    check(opened.string_graph(min_overlap=20, reduce=False), G, G.E)
    assert res.sequences() == G.seqs
    opened.close()
    # a golden with files: a duplicate and a contained record, no overlap between the kept ones
    entry = entry_named("shared_ends_duplicates")
    recs = golden_records(entry)
    text, _ = text_of(recs)
    words, hrows, drow = golden_outputs(entry)
    own = index_of(api, recs, s=4)
    opened = api.FMIndex.open(words, len(text), hrows, drow, own.samples(), sa_sample=4)
    G = Graph(rec_strings(recs), 8)
    assert sorted(G.state) == [0, 0, 0, 0, 1, 2]
    for fm in (own, opened):
        check(fm.string_graph(min_overlap=8), G, G.I)
    own.close(); opened.close()


def raw_call(fm, min_overlap, flags, capacity):
    L = fm._L
    state = np.full(fm.nrec, 9, dtype=np.uint8)
    offs = np.full(fm.nrec + 1, 77, dtype=np.uint64)
    edges = np.zeros(max(capacity, 1), dtype=np.dtype([("record", np.uint32), ("length", np.uint32)]))
    from debwt_amd import _lib
    rc = L.debwt_fm_string_graph(fm._h, min_overlap, flags, state.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                 offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                 edges.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmEdge)) if capacity else None, capacity)
    return rc, state, offs, edges[:capacity]


def test_errors_and_capacity(api, synth):
    strs, fm, graphs = synth
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
    assert raw_call(fm, 20, 0x80000001, 100)[0] == -1
    with pytest.raises(api.DebwtError):
        fm.string_graph(min_overlap=0)
    far = fm.string_graph(min_overlap=500)                     # longer than every record: states, no edges
    assert far.state.tolist() == G.state and len(far.edges) == 0 and not far.offsets.any()


def test_batches_do_not_change_results(api, synth, monkeypatch):
    strs, fm, graphs = synth
    for slots, hits in (("64", None), (None, "64"), ("64", "64")):
        for name, v in (("DEBWT_FM_OVERLAP_SLOTS", slots), ("DEBWT_FM_OVERLAP_HITS", hits)):
            monkeypatch.setenv(name, v) if v else monkeypatch.delenv(name, raising=False)
        base = None
        for L, reduce in ((1, False), (20, True), (1, True)):
            G = graphs[L]
            check(fm.string_graph(min_overlap=L, reduce=reduce), G, G.I if reduce else G.E)
            st = fm.graph_stats()
            assert st["edges"] == sum(len(l) for l in G.E)
            if L == 1 and base is None:
                base = st["launches"]
        assert base > 20                                       # many batches, or many expansions of one batch


# Every field of graph_stats() that is no time, on the synthetic reads at min_overlap 20, by (limits, reduce).  Recorded on
# an MI355X at the commit before the two graph builders shared one batch loop: they are sums and counts, and the batches
# depend on the input and the two limits alone.  A difference means a launch, a batch or a buffer changed.
_COUNTS = {"records": 436, "kept": 375, "duplicates": 9, "contained": 52, "hits": 3493, "edges": 2921, "edge_bytes": 23368}
PINNED = {
    (None, True): dict(_COUNTS, reducible=2549, lookups=2549, launches=12, scratch_bytes=594839),
    (None, False): dict(_COUNTS, reducible=0, lookups=0, launches=9, scratch_bytes=594839),
    ("64", True): dict(_COUNTS, reducible=2549, lookups=2549, launches=3001, scratch_bytes=7034),
    ("64", False): dict(_COUNTS, reducible=0, lookups=0, launches=2998, scratch_bytes=7034),
}


@pytest.mark.parametrize("limits", [None, "64"])
def test_stats_are_pinned(api, synth, monkeypatch, limits):
    strs, fm, _ = synth
    for name in ("DEBWT_FM_OVERLAP_SLOTS", "DEBWT_FM_OVERLAP_HITS"):
        monkeypatch.setenv(name, limits) if limits else monkeypatch.delenv(name, raising=False)
    got = {}
    for reduce in (True, False):
        fm.string_graph(min_overlap=20, reduce=reduce)
        got[limits, reduce] = {k: v for k, v in fm.graph_stats().items() if not k.startswith("ms_")}
        print("PINNED[%r, %r] = %r" % (limits, reduce, got[limits, reduce]))
    assert got == {k: v for k, v in PINNED.items() if k[0] == limits}


# ---- the reduction alone -----------------------------------------------------------------------------------------------

def reduce_on_gpu(api, fm, reclen, lists):
    offs, edges = flat(lists)
    keep = api.edges_reduce(fm, reclen, offs, np.array(edges, dtype=api._EDGE_DTYPE).reshape(-1))
    want = [0 if r else 1 for rl in reducible(lists, reclen) for r in rl]
    assert keep.tolist() == want
    st = fm.graph_stats()
    assert st["records"] == len(reclen) and st["edges"] == len(edges) and st["reducible"] == want.count(0)
    return want


def by_length(edges, rng=None):
    """lengths descending; one length's records descending, or shuffled: never in ascending order by design"""
    edges = sorted(edges, key=lambda e: (-e[1], -e[0]))
    if rng is not None:
        out = []
        for L in sorted({e[1] for e in edges}, reverse=True):
            grp = [e for e in edges if e[1] == L]
            out += [grp[int(i)] for i in rng.permutation(len(grp))]
        edges = out
    return edges


def crafted():
    """331 nodes of 1000 b.  Node 0 has 300 edges, two per length, to nodes 1..300.  Nodes 1..5 are witnesses with lists
    of 1, 63, 64, 65 and 300 entries: for a target k of node 0 the fitting length, or one base more for every third k;
    targets above 300 fill the longest list up.  Nodes 6.. have no edges."""
    nn = 331
    reclen = [1000] * nn
    L0 = {t: 800 - t // 2 for t in range(1, 301)}
    lists = [[] for _ in range(nn)]
    lists[0] = by_length([(t, L0[t]) for t in range(1, 301)])
    for j, size in ((1, 1), (2, 63), (3, 64), (4, 65), (5, 300)):
        ks = list(range(7, 7 + size))
        lists[j] = by_length([(k, reclen[j] - L0[j] + L0[k] + (1 if k % 3 == 0 else 0)) if k <= 300 else (k, 700 - k) for k in ks])
    return reclen, lists


def test_reduce_crafted_lists(api, synth):
    fm = synth[1]
    reclen, lists = crafted()
    assert [len(lists[j]) for j in range(7)] == [300, 1, 63, 64, 65, 300, 0]
    assert lists[0][1][0] > lists[0][2][0] and lists[0][1][1] == lists[0][2][1]     # a length group in descending record order
    want = reduce_on_gpu(api, fm, reclen, lists)
    red0 = reducible(lists, reclen)[0]
    by_target = {k: r for (k, _), r in zip(lists[0], red0)}
    assert by_target[7] and not by_target[6] and by_target[68] and not by_target[1] and not by_target[300]
    # witnesses at the first and at the last entry of a list: node 1's only entry, the last of node 2's 63 (k = 68)
    assert lists[1] == [(7, 1000 - 800 + 797)] and lists[2][-1] == (68, 1000 - 799 + 766) and lists[2][-2][1] > lists[2][-1][1]
    assert 100 < want.count(0) < 300
    # ties: 2 and 3 stand at one length in node 0's list, and 2 -> 3 whatever its length is no witness for 0 -> 3
    tie = [[(2, 50), (1, 50)], [(2, 99)], []]
    assert reduce_on_gpu(api, fm, [100, 100, 100], tie) == [1, 1, 1]
    # 0 -> 1 (40), 0 -> 2 (10): the witness is 1 -> 2 at 60 - 40 + 10 = 30; at 36, its longest, the edge stays
    assert reduce_on_gpu(api, fm, [60, 60, 60], [[(1, 40), (2, 10)], [(2, 30)], []]) == [1, 0, 1]
    assert reduce_on_gpu(api, fm, [60, 60, 60], [[(1, 40), (2, 10)], [(2, 36)], []]) == [1, 1, 1]
    assert reduce_on_gpu(api, fm, [60, 60, 60], [[(1, 40)], [], []]) == [1]              # sources with 1 and with 0 edges
    assert api.edges_reduce(fm, [60, 60], [0, 0, 0], np.zeros(0, dtype=api._EDGE_DTYPE)).tolist() == []
    assert api.edges_reduce(fm, [], [0], np.zeros(0, dtype=api._EDGE_DTYPE)).tolist() == []


def test_reduce_layout_with_noise(api, synth):
    """203 reads of 100 b laid on a line: every overlap is consistent, so all but the first edge of a source reduce;
    then every 5th length is changed by one and groups are shuffled"""
    fm = synth[1]
    rng = np.random.default_rng(8)
    pos = rng.permutation(3000)[:203].tolist()
    lists = [by_length([(k, 100 - (pos[k] - pos[i])) for k in range(203) if 0 < pos[k] - pos[i] <= 70]) for i in range(203)]
    want = reduce_on_gpu(api, fm, [100] * 203, lists)
    assert want.count(1) == sum(1 for l in lists if l)
    noisy = []
    for i, l in enumerate(lists):
        moved = [(k, L - 1 if (i + k) % 5 == 0 else L) for k, L in l]
        noisy.append(by_length(moved, rng))
    want = reduce_on_gpu(api, fm, [100] * 203, noisy)
    assert sum(1 for l in lists if l) < want.count(1) < len(want)


def test_reduce_errors(api, synth):
    fm = synth[1]
    E = api._EDGE_DTYPE

    def bad(reclen, offs, edges, word):
        with pytest.raises(api.DebwtError) as e:
            api.edges_reduce(fm, reclen, offs, np.array(edges, dtype=E).reshape(-1))
        assert e.value.args and word in str(e.value), str(e.value)

    r = [100, 100, 100]
    bad(r, [0, 2, 1, 2], [(1, 5), (2, 4)], "decrease")
    bad(r, [0, 1, 1, 1], [(3, 5)], "names node")
    bad(r, [0, 1, 1, 1], [(0, 5)], "own source")
    bad(r, [0, 2, 2, 2], [(1, 5), (2, 6)], "longer than")
    bad(r, [0, 2, 2, 2], [(1, 5), (1, 4)], "repeats")
    bad([100, 5, 100], [0, 1, 1, 1], [(1, 5)], "as long as")
    bad([5, 100, 100], [0, 1, 1, 1], [(1, 5)], "as long as")
    assert api.edges_reduce(fm, r, [0, 2, 2, 2], np.array([(1, 5), (2, 5)], dtype=E)).tolist() == [1, 1]


def test_reduce_list_with_mismatches(api):
    """overlaps_mm (K = 1, longest) of 200 mutated reads against themselves, self and flagged hits dropped"""
    strs = mutated_reads()[0][:200]
    fm = index_of(api, codes(strs), s=4)
    res = fm.overlaps_mm(strs, min_overlap=20, mismatches=1, longest=True)
    lists = []
    for i in range(len(strs)):
        h = res.hits(i)
        lists.append([(int(x["record"]), int(x["length"])) for x in h if int(x["record"]) != i and not int(x["flags"]) & 3])
    assert any(m for m in res.mismatches().tolist())
    want = reduce_on_gpu(api, fm, [len(s) for s in strs], lists)
    assert 0 < want.count(0) < len(want)
    fm.close()
