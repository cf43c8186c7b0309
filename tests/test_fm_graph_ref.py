"""The string graph's reference (string_graph_ref.py) and its host side, no GPU.  The reference alone must hold every
category the GPU comparison is meant to cover; debwt_fm_unitigs (api.unitigs) is compared with the reference's walk on
those graphs and on hand-made ones.

One category cannot come from records.  An edge i -> k that stays only because the fitting j -> k length is hidden behind a
longer j -> k overlap needs S_j's last L_jk bases to equal S_k's first L_jk with L_jk = want + s, s > 0.  S_i ends no later
than S_j in S_i's frame (L_ij < |S_j|) and agrees with S_j from S_j's start on, and S_k at that longer length starts
after S_j's start, so S_i's last L_ik + s bases lie inside S_j where S_j equals S_k: S_i -> S_k would overlap by L_ik + s,
and L_ik was not the longest.  With exact overlaps and the longest length per pair no such edge exists; the tests below
check that on periodic read sets, and cover the case where it does occur, on an edge list given to the reduction as
debwt_fm_edges_reduce takes them (filtered lists, lists with mismatches)."""
import numpy as np
import pytest

from overlap_ref import rand_dna, synthetic_reads
from string_graph_ref import (CONTAINED, DUPLICATE, KEPT, Graph, flat, reducible, repeat_reads, sampled_reads, tiling,
                              unitigs)


@pytest.fixture(scope="module")
def synth20():
    strs = synthetic_reads()
    return strs, Graph(strs, 20)


@pytest.fixture(scope="module")
def synth1():
    strs = synthetic_reads()
    return strs, Graph(strs, 1)


def hidden_edges(G):
    """irreducible edges i -> k for which some j in i's list overlaps k at the fitting length, though not at its longest"""
    out = []
    for i, l in enumerate(G.E):
        for (k, Lik), red in zip(l, G.red[i]):
            if red:
                continue
            for j, Lij in l:
                w = G.reclen[j] - Lij + Lik
                if j != k and Lij > Lik and G.min_overlap <= w < min(G.reclen[j], G.reclen[k]) and G.strs[j][-w:] == G.strs[k][:w]:
                    out.append((i, j, k))
    return out


def test_issue_figures(synth20, synth1):
    """the figures a separate prototype of the definitions gave on the same reads"""
    strs, G = synth20
    assert len(strs) == 436
    assert (G.state.count(KEPT), G.state.count(DUPLICATE), G.state.count(CONTAINED)) == (375, 9, 52)
    ne, nr = sum(len(l) for l in G.E), sum(sum(r) for r in G.red)
    assert (ne, nr, ne - nr, len(G.paths), max(len(s) for s in G.seqs)) == (2921, 2549, 372, 3, 2999)
    _, G1 = synth1
    assert G1.state == G.state                                 # states do not depend on min_overlap
    assert (sum(len(l) for l in G1.E), sum(sum(r) for r in G1.red), max(len(l) for l in G1.E)) == (46563, 3614, 148)


def test_reference_has_every_state(synth20):
    strs, G = synth20

    def kinds_of(strs, G):                                     # how each contained record lies in its longer records
        kinds = set()
        for i, s in enumerate(strs):
            if G.state[i] == CONTAINED:
                for t in strs:
                    if len(t) > len(s) and s in t:
                        kinds.add("prefix" if t.startswith(s) else "suffix" if t.endswith(s) else "inner")
        return kinds

    assert kinds_of(strs, G) >= {"prefix", "inner"}            # its only suffixes ("A" * 40 in "A" * 50) are prefixes too
    sampled = sampled_reads()
    assert kinds_of(sampled, Graph(sampled, 30)) == {"prefix", "suffix", "inner"}
    assert {KEPT, DUPLICATE, CONTAINED} == set(G.state)
    inner_only = [i for i, s in enumerate(strs) if G.state[i] == CONTAINED and
                  not any(len(t) > len(s) and (t.startswith(s) or t.endswith(s)) for t in strs)]
    assert inner_only                                          # contained, and no suffix-prefix overlap shows it


def test_reference_has_every_edge_kind(synth20, synth1):
    _, G = synth20
    flat_red = [r for rl in G.red for r in rl]
    assert any(flat_red) and not all(flat_red)
    _, G1 = synth1
    assert max(len(l) for l in G1.E) > 64
    assert any(len({L for _, L in l}) < len(l) for l in G1.E)      # several records at one length
    for l in G.E + G1.E:
        assert l == sorted(l, key=lambda e: (-e[1], e[0])) and len({j for j, _ in l}) == len(l)


def test_no_hidden_witness_among_records(synth20, synth1):
    assert hidden_edges(synth20[1]) == [] and hidden_edges(synth1[1]) == []
    rng = np.random.default_rng(3)
    for unit in ("AC", "ACG", "AAC", "ACGT"):                  # reads of a tandem repeat with unique flanks
        g = rand_dna(rng, 40) + unit * 30 + rand_dna(rng, 40)
        reads = [g[a:a + int(rng.integers(25, 50))] for a in range(0, len(g) - 50, 3)]
        G = Graph(reads, 8)
        assert any(any(r) for r in G.red) and any(len({L for _, L in l}) > 1 for l in G.E)
        assert hidden_edges(G) == []


def test_hidden_witness_in_a_given_list():
    """0 -> 1 (40), 0 -> 2 (10), |S_1| = 60: the witness is 1 -> 2 at 60 - 40 + 10 = 30.  A list that holds 1 -> 2 only at 36
    (its longest, as DEBWT_FM_OVERLAP_LONGEST leaves it) keeps 0 -> 2; one that holds it at 30 drops it."""
    reclen = [60, 60, 60]
    assert reducible([[(1, 40), (2, 10)], [(2, 36)], []], reclen) == [[False, False], [False], []]
    assert reducible([[(1, 40), (2, 10)], [(2, 30)], []], reclen) == [[False, True], [False], []]
    assert reducible([[(1, 40), (2, 40)], [(2, 60)], []], reclen) == [[False, False], [False], []]   # a tie is no witness


def test_reference_unitigs_and_sequences(synth20):
    _, G = synth20
    assert G.circular == [0, 0, 0] and sorted(len(s) for s in G.seqs)[-1] == 2999
    g, reads = tiling(1, 2000, 60, 5)
    T = Graph(reads, 30)
    assert T.seqs == [g] and T.circular == [0] and len(T.paths[0]) == len(reads)
    g, reads = tiling(2, 1500, 60, 5, circle=True)
    C = Graph(reads, 30)
    assert C.circular == [1] and len(C.seqs[0]) == 1500 and C.seqs[0] in g + g and C.paths[0][0] == 0
    _, reads = repeat_reads()
    B = Graph(reads, 30)
    assert len(B.paths) > 1 and max(len(l) for l in B.I) == 2          # branch-bounded unitigs
    S = Graph(sampled_reads(), 30)
    assert {KEPT, DUPLICATE, CONTAINED} == set(S.state)
    single = Graph(["ACGTACGTAA", "TTTTTGGGGG", "ACGTACGTAA"], 5)
    assert single.paths == [[0], [1]] and single.circular == [0, 0] and single.seqs == ["ACGTACGTAA", "TTTTTGGGGG"]


def api_unitigs(state, lists):
    from debwt_amd import api
    offs, edges = flat(lists)
    uoff, mem, circ = api.unitigs(state, offs, np.array(edges, dtype=api._EDGE_DTYPE))
    paths = [[int(x) for x in mem[int(uoff[u]):int(uoff[u + 1])]] for u in range(len(circ))]
    assert len(uoff) == len(circ) + 1 and int(uoff[0]) == 0
    return paths, [int(c) for c in circ]


def test_unitigs_against_the_reference(synth20, synth1):
    graphs = [synth20[1], synth1[1], Graph(tiling(1, 2000, 60, 5)[1], 30), Graph(tiling(2, 1500, 60, 5, circle=True)[1], 30),
              Graph(repeat_reads()[1], 30), Graph(sampled_reads(), 30)]
    for G in graphs:
        for lists in (G.I, G.E):
            assert api_unitigs(G.state, lists) == unitigs(G.state, lists)


HAND = {
    "two cycles": ([0] * 6, [[(2, 5)], [(3, 5)], [(4, 5)], [(5, 5)], [(0, 5)], [(1, 5)]]),
    "a cycle with a tail": ([0] * 5, [[(1, 5)], [(2, 5)], [(3, 5)], [(1, 4)], []]),
    "indeg 2": ([0] * 4, [[(2, 5)], [(2, 6)], [(3, 5)], []]),
    "outdeg 1 into indeg 2": ([0] * 5, [[(1, 5)], [(3, 5)], [(3, 5)], [(4, 5)], []]),
    "a chain that starts at its highest node": ([0] * 4, [[], [(0, 5)], [(1, 5)], [(2, 5)]]),
    "a cycle whose lowest node comes late": ([0] * 5, [[], [], [(4, 5)], [(2, 5)], [(3, 5)]]),
    "a self edge": ([0] * 2, [[(0, 3)], []]),
    "nodes that are not kept": ([0, 1, 2, 0, 0], [[(3, 5)], [], [], [(4, 5)], []]),
    "empty graph": ([], []),
    "no edges": ([0, 2, 0], [[], [], []]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_unitigs_hand_made(name):
    state, lists = HAND[name]
    want = unitigs(state, lists)
    assert api_unitigs(state, lists) == want
    if name == "two cycles":
        assert want == ([[0, 2, 4], [1, 3, 5]], [1, 1])
    if name == "a cycle with a tail":                          # node 1 has two predecessors: no link enters it
        assert want == ([[0], [1, 2, 3], [4]], [0, 0, 0])
    if name == "a chain that starts at its highest node":
        assert want == ([[3, 2, 1, 0]], [0])
    if name == "a cycle whose lowest node comes late":
        assert want == ([[0], [1], [2, 4, 3]], [0, 0, 1])
    if name == "nodes that are not kept":
        assert want == ([[0, 3, 4]], [0])


def test_unitigs_errors():
    from debwt_amd import api
    e = np.array([(1, 5)], dtype=api._EDGE_DTYPE)
    with pytest.raises(api.DebwtError):
        api.unitigs([0, 1], [0, 1, 1], e)                      # an edge to a node that is not kept
    with pytest.raises(api.DebwtError):
        api.unitigs([1, 0], [0, 1, 1], e)                      # an edge from one
    with pytest.raises(api.DebwtError):
        api.unitigs([0, 0], [0, 1, 1], np.array([(2, 5)], dtype=api._EDGE_DTYPE))
    with pytest.raises(api.DebwtError):
        api.unitigs([0, 0], [1, 0, 1], e)
    with pytest.raises(ValueError):
        api.unitigs([0, 0], [0, 1], e)
