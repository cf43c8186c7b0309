"""The reference of the graph cleaning tests (graph_clean_ref.py, definition 6 of debwt_hip.h) pinned on the shared read
set -- a 2 kb tiling with five end-error reads and six reads of a second allele, on one strand and on both -- and
debwt_fm_edges_compact (host only) against a list comprehension.  No GPU."""
import numpy as np
import pytest

import bigraph_ref as bg
import graph_clean_ref as gc
import string_graph_ref as sg
from overlap_ref import revcomp


@pytest.fixture(scope="module")
def single():
    g, reads = gc.error_reads()
    return g, reads, sg.Graph(reads, 40)


@pytest.fixture(scope="module")
def double():
    g, reads = gc.error_reads()
    reads = bg.stranded(reads, 3)
    return g, reads, sg.Graph(bg.doubled(reads), 40)


def test_single_strand(single):
    g, reads, G = single
    assert len(reads) == 395 and len(G.paths) == 14
    state, lists, rounds = gc.clean(G.state, G.I, 3, 16, 8)
    assert (state.count(gc.CLIPPED), state.count(gc.POPPED), rounds) == (5, 6, 2)
    paths, circ = sg.unitigs(state, lists)
    assert len(paths) == 1 and circ == [0]
    assert sg.sequences(reads, lists, paths, circ) == [g]
    full = gc.clean_full(G.state, G.I, 3, 16, 8)
    assert (full["tips"], full["tip_nodes"], full["bubbles"], full["bubble_nodes"]) == (5, 5, 1, 6)
    # the edges left are those between the nodes left, in their order
    assert lists == [[e for e in l if state[u] == 0 and state[e[0]] == 0] for u, l in enumerate(G.I)]


def test_single_strand_short_bubble_bound(single):
    _, _, G = single
    state, lists, _ = gc.clean(G.state, G.I, 3, 4, 8)             # the allele's branch has 6 nodes: it stays
    assert (state.count(gc.CLIPPED), state.count(gc.POPPED)) == (5, 0)
    assert len(sg.unitigs(state, lists)[0]) == 4


def test_both_strands(double):
    g, reads, G = double
    assert len(bg.unitigs_both(G.state, G.I)[0]) == 14
    state, lists, rounds = gc.clean(G.state, G.I, 3, 16, 8, mirrored=True)
    assert (state.count(gc.CLIPPED), state.count(gc.POPPED), rounds) == (10, 12, 2)
    assert all((state[v] == 0) == (state[v ^ 1] == 0) for v in range(len(state)))
    have = {(u, e[0]) for u, l in enumerate(lists) for e in l}
    assert all((v ^ 1, u ^ 1) in have for u, v in have)
    paths, circ = bg.unitigs_both(state, lists)
    assert len(paths) == 1
    assert bg.sequences_both(reads, lists, paths, circ)[0] in (g, revcomp(g))
    state, _, _ = gc.clean(G.state, G.I, 3, 4, 8, mirrored=True)
    assert (state.count(gc.CLIPPED), state.count(gc.POPPED)) == (10, 0)


def test_rounds_and_phases_can_be_switched_off(single):
    _, _, G = single
    state, _, rounds = gc.clean(G.state, G.I, 0, 16, 8)            # bubbles only
    assert (state.count(gc.CLIPPED), state.count(gc.POPPED), rounds) == (0, 6, 2)
    state, _, rounds = gc.clean(G.state, G.I, 3, 0, 8)             # tips only
    assert (state.count(gc.CLIPPED), state.count(gc.POPPED), rounds) == (5, 0, 2)
    state, _, rounds = gc.clean(G.state, G.I, 3, 16, 1)
    assert (state.count(gc.CLIPPED), state.count(gc.POPPED), rounds) == (5, 6, 1)


def test_edges_compact_host():
    from debwt_amd import api
    rng = np.random.default_rng(12)
    for nn in (0, 1, 7, 300):
        deg = rng.integers(0, 5, size=nn)
        offs = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
        ne = int(offs[-1])
        edges = np.zeros(ne, dtype=api._EDGE_DTYPE)
        edges["record"] = rng.integers(0, max(nn, 1), size=ne)
        edges["length"] = rng.integers(1, 100, size=ne)
        keep = (rng.random(ne) < 0.6).astype(np.uint8)
        o, e = api.edges_compact(offs, edges, keep)
        want = [[tuple(edges[k].tolist()) for k in range(int(offs[i]), int(offs[i + 1])) if keep[k]] for i in range(nn)]
        wo, we = sg.flat(want)
        assert o.tolist() == wo and [tuple(x) for x in e.tolist()] == we
    with pytest.raises(api.DebwtError):
        api.edges_compact(np.array([0, 2, 1], dtype=np.uint64), np.zeros(2, dtype=api._EDGE_DTYPE), np.ones(2, dtype=np.uint8))
    assert api.NODE_CLIPPED == gc.CLIPPED == 3 and api.NODE_POPPED == gc.POPPED == 4
