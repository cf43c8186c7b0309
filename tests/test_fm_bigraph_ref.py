"""The string graph over both strands, no GPU: what follows from applying string_graph_ref.Graph to the doubled collection
(the state fold rule, mirror symmetry of E and of the irreducible graph, every kept read in exactly one oriented unitig)
on stranded read sets with crafted corners, and debwt_fm_unitigs_both (api.unitigs_both) against definition 4b taken
literally, on those graphs, on hand-made ones and on bad input; debwt_fm_unitigs (api.unitigs) on the same graphs against
definition 4, which the rules of 4b must not reach."""
import numpy as np
import pytest

from bigraph_ref import (all_unitigs_both, crafted, doubled, fold_states, is_selfrc, mirror, sequences_both, stranded,
                         unitigs_both)
from overlap_ref import revcomp, synthetic_reads
from string_graph_ref import KEPT, Graph, flat, repeat_reads, tiling
from string_graph_ref import unitigs as plain_unitigs


@pytest.fixture(scope="module")
def crafted_set():
    strs, names = crafted(stranded(synthetic_reads(), 7))
    return strs, names, {L: Graph(doubled(strs), L) for L in (20, 41)}


def other_sets():
    return [(stranded(tiling(1, 2000, 60, 5)[1], 3), 30), (stranded(tiling(2, 1500, 60, 5, circle=True)[1], 4), 30),
            (stranded(repeat_reads()[1], 5), 30)]


def mirror_node(state, v):
    return v if is_selfrc(state, v) else v ^ 1


def asymmetric(state, lists):
    have = {(u, v, L) for u, l in enumerate(lists) for v, L in l}
    return [(u, v, L) for u, v, L in have if (mirror_node(state, v), mirror_node(state, u), L) not in have]


def api_unitigs_both(state, lists):
    from debwt_amd import api
    offs, edges = flat(lists)
    uoff, mem, circ = api.unitigs_both(state, offs, np.array(edges, dtype=api._EDGE_DTYPE).reshape(-1))
    assert len(uoff) == len(circ) + 1 and int(uoff[0]) == 0
    return [[int(x) for x in mem[int(uoff[u]):int(uoff[u + 1])]] for u in range(len(circ))], [int(c) for c in circ]


def check_graph(strs, G):
    assert G.state == fold_states(strs)
    assert asymmetric(G.state, G.E) == [] and asymmetric(G.state, G.I) == []
    every = all_unitigs_both(G.state, G.I)
    keys = {(tuple(p), c) for p, c in every}
    assert all((tuple(mirror(G.state, p, c)), c) in keys for p, c in every)      # unitigs come in mirror pairs
    paths, circ = unitigs_both(G.state, G.I)
    reads = sorted(v >> 1 for p in paths for v in p)
    assert reads == [r for r in range(len(strs)) if G.state[2 * r] == KEPT]       # each kept read once, in one orientation
    assert [p[0] for p in paths] == sorted(p[0] for p in paths)
    assert api_unitigs_both(G.state, G.I) == (paths, circ)
    assert api_unitigs_both(G.state, G.E) == unitigs_both(G.state, G.E)
    return paths, circ


def check_figures(G):
    """The 436 stranded synthetic reads keep the states test_fm_graph_ref.py pins for the forward set (a strand changes
    no state: the fold rule, checked in check_graph), and the edge kinds pair up as the mirror says."""
    st = G.state[0:2 * 436:2]
    assert (st.count(0), st.count(1), st.count(2)) == (375, 9, 52)
    kinds = [0, 0, 0, 0]
    for u, l in enumerate(G.E):
        for v, _ in l:
            kinds[2 * (u & 1) + (v & 1)] += 1
    # the mirror of a ++ edge is a -- edge (the self-rc reads here have no edges); the mirror of (i+ -> j-) is (j+ -> i-),
    # of its own kind, and its own mirror when i == j: the +- and the -+ edges pair up among themselves
    own = [sum(1 for u in range(o, len(G.E), 2) for v, _ in G.E[u] if v == u ^ 1) for o in (0, 1)]
    assert kinds[0] == kinds[3] and (kinds[1] - own[0]) % 2 == 0 and (kinds[2] - own[1]) % 2 == 0
    assert kinds[1] != kinds[2] and min(kinds) > 1000          # about a quarter of each kind


@pytest.mark.parametrize("min_overlap", [20, 41])
def test_crafted_set(crafted_set, min_overlap):
    strs, names, graphs = crafted_set
    G = graphs[min_overlap]
    check_graph(strs, G)
    r = names["selfrc"]
    assert G.state[2 * r:2 * r + 2] == [0, 1] and G.E[2 * r + 1] == []
    assert G.state[2 * names["selfrc_contained"]:2 * names["selfrc_contained"] + 2] == [2, 1]
    assert G.state[2 * names["rc_duplicate"]] == 1 and G.state[2 * names["rc_inner"]] == 2
    a, b, m = names["tail_a"], names["tail_b"], names["own_mirror"]
    tails = [e for e in G.E[2 * a] if e[0] == 2 * b + 1]
    own = [e for e in G.E[2 * m] if e[0] == 2 * m + 1]
    if min_overlap == 20:
        assert tails == [(2 * b + 1, 20)] and (2 * a + 1, 20) in G.E[2 * b]       # tail to tail, and its mirror
        assert own == [(2 * m + 1, 24)]                                            # a read that overlaps its own mirror
        check_figures(G)
    else:
        assert tails == [] and own == []
    for x, y in (("short_a", "short_b"), ("mismatch_src", "mismatch"), ("early_src", "early")):
        assert not [e for e in G.E[2 * names[x]] if e[0] >> 1 == names[y]]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_other_sets(which):
    strs, L = other_sets()[which]
    G = Graph(doubled(strs), L)
    paths, circ = check_graph(strs, G)
    seqs = sequences_both(strs, G.I, paths, circ)
    if which == 0:
        g = tiling(1, 2000, 60, 5)[0]
        assert len(paths) == 1 and circ == [0] and seqs[0] in (g, revcomp(g))
    if which == 1:
        g = tiling(2, 1500, 60, 5, circle=True)[0]
        assert circ == [1] and len(seqs[0]) == 1500 and (seqs[0] in g + g or revcomp(seqs[0]) in g + g)
    if which == 2:
        assert len(paths) > 1


# nodes 2r + o; a self-rc read has state (0, 1)
HAND = {
    # 0 -> 3 is the mirror of 2 -> 1: two reads, one link each way; both unitigs are mirrors of each other
    "a mirror pair": ([0, 0, 0, 0], [[(3, 5)], [], [(1, 5)], []]),
    # 0 -> 1 leads to the source's own mirror: no link, though in and out degree are 1
    "a link to the own mirror": ([0, 0], [[(1, 5)], []]),
    # read 1 is self-rc (node 2 only): 0 -> 2 and its mirror 2 -> 1 are links of definition 4 and would chain 0, 2, 1
    "through a self-rc node": ([0, 0, 0, 1], [[(2, 5)], [], [(1, 5)], []]),
    "a chain and its mirror": ([0] * 6, [[(2, 5)], [], [(4, 5)], [(1, 5)], [], [(3, 5)]]),
    # a cycle over reads 0, 1, 2 as + + -, and its mirror 4 -> 3 -> 1 -> 4
    "a cycle and its mirror": ([0] * 6, [[(2, 5)], [(4, 5)], [(5, 5)], [(1, 5)], [(3, 5)], [(0, 5)]]),
    "nodes that are not kept": ([0, 0, 2, 2, 1, 1, 0, 0], [[(6, 5)], [], [], [], [], [], [], [(1, 5)]]),
    "empty graph": ([], []),
    "no edges": ([0, 0, 0, 1], [[], [], [], []]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_unitigs_both_hand_made(name):
    state, lists = HAND[name]
    assert asymmetric(state, lists) == []
    want = unitigs_both(state, lists)
    assert api_unitigs_both(state, lists) == want
    if name == "a mirror pair":
        assert want == ([[0, 3]], [0])
    if name == "a link to the own mirror":
        assert want == ([[0]], [0])
    if name == "through a self-rc node":
        assert want == ([[0], [2]], [0, 0])
    if name == "a chain and its mirror":
        assert want == ([[0, 2, 4]], [0])
    if name == "a cycle and its mirror":
        assert want == ([[0, 2, 5]], [1])
    if name == "nodes that are not kept":
        assert want == ([[0, 6]], [0])
    if name == "no edges":
        assert want == ([[0], [2]], [0, 0])


def api_unitigs(state, lists):
    from debwt_amd import api
    offs, edges = flat(lists)
    uoff, mem, circ = api.unitigs(state, offs, np.array(edges, dtype=api._EDGE_DTYPE).reshape(-1))
    assert len(uoff) == len(circ) + 1 and int(uoff[0]) == 0
    return [[int(x) for x in mem[int(uoff[u]):int(uoff[u + 1])]] for u in range(len(circ))], [int(c) for c in circ]


def test_strand_zero_unitigs_keep_the_plain_rule(crafted_set):
    """api.unitigs on a graph of 2 nrec nodes is definition 4 as string_graph_ref has it: none of the rules of
    unitigs_both (no link to v ^ 1, none at a self-rc read, one of a mirror pair) reaches the strand-0 call."""
    for name in sorted(HAND):
        state, lists = HAND[name]
        plain = plain_unitigs(state, lists)
        assert api_unitigs(state, lists) == plain, name
        if name in ("a link to the own mirror", "through a self-rc node"):
            assert plain != api_unitigs_both(state, lists), name
    assert plain_unitigs(*HAND["a link to the own mirror"]) == ([[0, 1]], [0])
    assert plain_unitigs(*HAND["through a self-rc node"]) == ([[0, 2, 1]], [0])
    for G in crafted_set[2].values():
        assert api_unitigs(G.state, G.I) == (G.paths, G.circular)


def test_unitigs_both_errors():
    from debwt_amd import api
    E = api._EDGE_DTYPE
    e = np.array([(1, 5)], dtype=E)
    with pytest.raises(api.DebwtError):
        api.unitigs_both([0, 1], [0, 1, 1], e)                 # an edge to a node that is not kept
    with pytest.raises(api.DebwtError):
        api.unitigs_both([1, 0], [0, 1, 1], e)                 # an edge from one
    with pytest.raises(api.DebwtError):
        api.unitigs_both([0, 0], [0, 1, 1], np.array([(2, 5)], dtype=E))      # a target past the nodes
    with pytest.raises(api.DebwtError):
        api.unitigs_both([0, 0], [1, 0, 1], e)                 # decreasing offsets
    with pytest.raises(api.DebwtError):
        api.unitigs_both([0, 0, 0], [0, 1, 1, 1], e)           # an odd number of nodes
    with pytest.raises(ValueError):
        api.unitigs_both([0, 0], [0, 1], e)
    assert api.unitigs(np.array([0, 0, 0]), [0, 1, 1, 1], e)[1].tolist() == [0, 1, 2]     # the strand-0 call takes it
