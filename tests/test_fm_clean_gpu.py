"""Graph cleaning on the GPU (debwt_fm_graph_clean; api.graph_clean, GraphResult.clean, BiGraphResult.clean) against
definition 6 taken literally in graph_clean_ref.py: state_out, edge_keep, rounds and the four counters compared exactly on
the shared read set with errors (one strand and both, then unitigs and sequences), one hand-made graph per corner of the
definition, random digraphs, random mirrored digraphs, a graph of 70,000 nodes, each phase alone, and every error."""
import ctypes

import numpy as np
import pytest

import bigraph_ref as bg
import graph_clean_ref as gc
import string_graph_ref as sg
from overlap_ref import codes, revcomp
from test_fm_search_gpu import index_of

pytestmark = pytest.mark.gpu

CORNERS = gc.corner_graphs()


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


@pytest.fixture(scope="module")
def recipe(api):
    """(g, reads, their index): the index also serves the tests that bring their own graph"""
    g, reads = gc.error_reads()
    fm = index_of(api, codes(reads))
    yield g, reads, fm
    fm.close()


@pytest.fixture(scope="module")
def stranded(api):
    """the same with every read on a random strand"""
    g, reads = gc.error_reads()
    reads = bg.stranded(reads, 3)
    fm = index_of(api, codes(reads))
    yield g, reads, fm
    fm.close()


def arrays(api, lists):
    offs, edges = sg.flat(lists)
    return np.array(offs, dtype=np.uint64), np.array([(e[0], e[1]) for e in edges], dtype=api._EDGE_DTYPE)


def check(api, fm, state, lists, T, B, R, mirrored):
    """the call against the reference; returns the reference's result"""
    ref = gc.clean_full(state, lists, T, B, R, mirrored)
    offs, edges = arrays(api, lists)
    out, keep = api.graph_clean(fm, state, offs, edges, T, B, R, mirrored=mirrored)
    st = fm.clean_stats()
    got = {k: st[k] for k in ("rounds", "tips", "tip_nodes", "bubbles", "bubble_nodes")}
    print(got, "removed", sum(1 for a, b in zip(ref["state"], state) if a != b))
    assert out.tolist() == ref["state"]
    assert keep.tolist() == [int(k) for kl in ref["keep"] for k in kl]
    assert got == {k: ref[k] for k in got}
    assert st["nodes"] == len(state) and st["edges"] == len(edges)
    if len(edges):
        assert st["launches"] >= 2 + 3 * st["rounds"] and st["ms_clean"] > 0 and st["ms_wall"] > 0
        assert st["steps"] >= st["tip_nodes"] + st["bubble_nodes"]
    return ref


def test_read_set_one_strand(api, recipe):
    g, reads, fm = recipe
    G = sg.Graph(reads, 40)
    res = fm.string_graph(min_overlap=40)
    assert len(res.unitigs()[2]) == len(G.paths) == 14
    ref = check(api, fm, G.state, G.I, 3, 16, 8, False)
    assert (ref["state"].count(3), ref["state"].count(4), ref["rounds"]) == (5, 6, 2)
    cl = res.clean(max_tip=3)
    assert type(cl) is api.GraphResult and cl.reduced and cl.index is fm
    state, lists, _ = gc.clean(G.state, G.I, 3, 16, 8)
    offs, edges = sg.flat(lists)
    assert cl.state.tolist() == state and cl.offsets.tolist() == offs
    assert [tuple(int(x) for x in e) for e in cl.edges.tolist()] == edges
    paths, circ = sg.unitigs(state, lists)
    uoff, mem, c = cl.unitigs()
    assert len(c) == 1 and mem.tolist() == paths[0] and c.tolist() == circ
    assert cl.sequences() == sg.sequences(reads, lists, paths, circ) == [g]
    assert res.state.tolist() == G.state                        # the graph cleaned is left as it was
    with pytest.raises(ValueError):
        fm.string_graph(min_overlap=40, reduce=False).clean()


def test_read_set_both_strands(api, stranded):
    g, reads, fm = stranded
    G = sg.Graph(bg.doubled(reads), 40)
    res = fm.string_graph_both(min_overlap=40)
    assert len(res.unitigs()[2]) == 14
    ref = check(api, fm, G.state, G.I, 3, 16, 8, True)
    assert (ref["state"].count(3), ref["state"].count(4), ref["rounds"]) == (10, 12, 2)
    cl = res.clean(max_tip=3)
    assert type(cl) is api.BiGraphResult
    state, lists, _ = gc.clean(G.state, G.I, 3, 16, 8, mirrored=True)
    assert cl.state.tolist() == state and cl.offsets.tolist() == sg.flat(lists)[0]
    assert all((state[v] == 0) == (state[v ^ 1] == 0) for v in range(len(state)))
    paths, circ = bg.unitigs_both(state, lists)
    uoff, mem, c = cl.unitigs()
    assert len(c) == 1 and mem.tolist() == paths[0]
    seqs = cl.sequences()
    assert seqs == bg.sequences_both(reads, lists, paths, circ) and seqs[0] in (g, revcomp(g))
    short = res.clean(max_tip=3, max_bubble=4)                  # the allele's branch has 6 nodes
    assert (short.state.tolist().count(api.NODE_CLIPPED), short.state.tolist().count(api.NODE_POPPED)) == (10, 0)


@pytest.mark.parametrize("name", sorted(CORNERS))
def test_corner(api, recipe, name):
    state, lists, T, B, R, mirrored, expect = CORNERS[name]
    assert len(state) <= 20
    ref = check(api, recipe[2], state, lists, T, B, R, mirrored)
    assert {v: s for v, (s, s0) in enumerate(zip(ref["state"], state)) if s != s0} == expect
    if T and B:                                                 # each phase alone
        check(api, recipe[2], state, lists, 0, B, R, mirrored)
        check(api, recipe[2], state, lists, T, 0, R, mirrored)


def test_tip_that_a_popped_bubble_leaves(api, recipe):
    state, lists, T, B, _, _, _ = CORNERS["tip_after_pop"]
    assert check(api, recipe[2], state, lists, T, B, 8, False)["rounds"] == 3
    assert check(api, recipe[2], state, lists, T, B, 2, False)["rounds"] == 2
    one = check(api, recipe[2], state, lists, T, B, 1, False)
    assert one["rounds"] == 1 and one["state"].count(3) == 0 and one["state"].count(4) == 1


def test_random_digraphs(api, recipe):
    rng = np.random.default_rng(21)
    tips = pops = 0
    for _ in range(200):
        state, lists = gc.random_graph(rng)
        ref = check(api, recipe[2], state, lists, int(rng.integers(1, 6)), int(rng.integers(1, 9)), 8, False)
        tips += ref["tips"] > 0
        pops += ref["bubbles"] > 0
    assert tips > 100 and pops > 20                             # the graphs do exercise both phases


def test_random_mirrored_digraphs(api, recipe):
    rng = np.random.default_rng(22)
    pops = 0
    for _ in range(60):
        state, lists = gc.random_mirrored_graph(rng)
        ref = check(api, recipe[2], state, lists, int(rng.integers(1, 6)), int(rng.integers(1, 9)), 8, True)
        s = ref["state"]
        assert all((s[v] == 0) == (s[v ^ 1] == 0) for v in range(len(s)))
        pops += ref["bubbles"] > 0
    assert pops > 5


def test_seventy_thousand_nodes(api, recipe):
    state, lists = gc.long_chains()
    assert len(state) >= 70000
    ref = check(api, recipe[2], state, lists, 3, 16, 8, False)
    assert ref["tips"] > 900 and ref["tip_nodes"] > ref["tips"] and ref["rounds"] == 2
    offs, _ = sg.flat(lists)
    # sibling edges of one junction on both sides of a wave's last lane
    assert any(offs[u + 1] - offs[u] == 2 and offs[u] % 64 == 63 for u in range(len(state)))


def test_no_nodes_and_no_edges(api, recipe):
    fm = recipe[2]
    out, keep = api.graph_clean(fm, [], [0], np.zeros(0, dtype=api._EDGE_DTYPE))
    assert len(out) == 0 and len(keep) == 0
    out, keep = api.graph_clean(fm, [0, 1, 2, 0], [0, 0, 0, 0, 0], np.zeros(0, dtype=api._EDGE_DTYPE))
    assert out.tolist() == [0, 1, 2, 0] and len(keep) == 0 and fm.clean_stats()["rounds"] == 1


def test_errors(api, recipe):
    fm = recipe[2]
    state, lists = CORNERS["bubble_unequal"][:2]
    offs, edges = arrays(api, lists)

    def fails(why, st=state, o=offs, e=edges, **kw):
        with pytest.raises(api.DebwtError) as x:
            api.graph_clean(fm, st, o, e, **kw)
        assert x.value.code == -1 and "debwt_fm_graph_clean" in str(x.value) and why in str(x.value), str(x.value)

    fails("both 0", max_tip=0, max_bubble=0)
    fails("max_rounds", max_rounds=0)
    fails("odd number of nodes", mirrored=True)
    o = offs.copy()
    o[2], o[3] = o[3], o[2] - 1
    fails("offsets must not decrease", o=o)
    e = edges.copy()
    e["record"][2] = len(state)
    fails(f"names node {len(state)} of {len(state)}", e=e)
    dead = list(state)
    dead[4] = 2                                                 # 1 -> 4 -> 5
    fails("leads to node 4, which is not alive", st=dead)
    dead = list(state)
    dead[0] = 1
    fails("leaves a node that is not alive", st=dead)
    # unknown flags and 2^32 nodes, through the C interface
    from debwt_amd import _lib
    u8p, edgep = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(_lib.DebwtFmEdge)
    s8 = np.array(state, dtype=np.uint8)
    out, keep = np.zeros(len(state), dtype=np.uint8), np.zeros(len(edges), dtype=np.uint8)

    def raw(opts, nn):
        return fm._L.debwt_fm_graph_clean(fm._h, s8.ctypes.data_as(u8p), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                          edges.ctypes.data_as(edgep), nn, ctypes.byref(opts), out.ctypes.data_as(u8p),
                                          keep.ctypes.data_as(u8p))

    opts = _lib.DebwtFmCleanOpts()
    fm._L.debwt_fm_clean_defaults(ctypes.byref(opts))
    assert (opts.max_tip, opts.max_bubble, opts.max_rounds, opts.flags) == (4, 16, 8, 0)
    assert raw(opts, len(state)) == 0 and out.tolist() == gc.clean_full(state, lists, 4, 16, 8)["state"]
    assert raw(opts, 1 << 32) == -1 and b"2^32 nodes" in fm._L.debwt_fm_last_error(fm._h)
    opts.flags = 2
    assert raw(opts, len(state)) == -1 and b"unknown flags" in fm._L.debwt_fm_last_error(fm._h)
