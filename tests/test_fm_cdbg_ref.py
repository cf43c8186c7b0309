"""Definition 13 on the CPU (cdbg_ref.py): the dictionary brute force against the interval rules over esa_ref.Esa on every
geometry case, the three facts and the edge property on each, the hand examples of the definition, and the inputs the GPU
tests rest on with the figures the definition gives for them."""
import numpy as np
import pytest

import cdbg_ref as CR
import esa_ref as ER
import fm_definition as F

CASES = F.geometry_cases()
KS = (1, 2, 3, 5, 8)


def codes(strs):
    return [np.array([F.ACGT.index(c) for c in s], dtype=np.uint8) for s in strs]


@pytest.mark.parametrize("name", list(CASES))
def test_geometry_cases(name):
    E = ER.of_case(name)
    strs = F.strings(CASES[name])
    for k in KS:
        G = CR.from_esa(E, k)
        CR.same_graph(G, CR.brute(strs, k), rows=False)            # assemble() asserts the edge property in both
        CR.facts(G, E, strs)
        CR.same_graph(G, CR.from_esa(E, k, max_lcp=k + 1))          # a build capped at k + 1 tells lcp = k from lcp > k
        assert G.strings() == CR.brute(strs, k).strings()
        for s, u in zip(G.strings(), G.unitigs):                    # row_lo is the first row of the first k-mer
            assert E.sym[int(E.sa[int(u["row_lo"])]):][:k].tolist() == [F.ACGT.index(c) for c in s[:k]]


def test_what_the_cases_are_here_for():
    for name in ("ones_600", "short_1to3_x500"):                    # most or all rows are pieces that are no node
        G = CR.from_esa(ER.of_case(name), 5)
        assert G.sizes() == (0, 0, 0) and G.counts["nodes"] == 0
    assert CR.from_esa(ER.of_case("short_1to3_x500"), 3).counts["nodes"] > 0
    for name in ("all_T_x3", "homopolymer_only_one_record"):        # one node with a wide interval and a self edge
        G = CR.from_esa(ER.of_case(name), 8)
        assert G.strings() in (["T" * 8], ["G" * 8]) and G.edges.tolist() == [(0, 0)] and G.unitigs["flags"][0] == 0
        assert 380 <= G.unitigs["kmer_count"][0] <= 500
    assert CR.from_esa(ER.of_case("n2"), 1).strings() == ["A"] and CR.from_esa(ER.of_case("n2"), 2).sizes() == (0, 0, 0)
    G = CR.from_esa(ER.of_case("dup_40x20"), 8)
    assert (G.unitigs["kmer_count"] % 20 == 0).all()


def hand(strs, k):
    E = ER.Esa(codes(strs))
    G = CR.from_esa(E, k)
    CR.same_graph(G, CR.brute(strs, k), rows=False)
    CR.facts(G, E, strs)
    return G


def test_hand_examples():
    G = hand(["ACGTACGTACGT"], 4)
    assert G.strings() == ["ACGTACG"] and G.unitigs["nodes"].tolist() == [4] and G.unitigs["kmer_count"].tolist() == [9]
    assert G.unitigs["flags"].tolist() == [CR.CIRCULAR] and G.edges.tolist() == [(0, 0)]
    G = hand(["AAAAAAA"], 3)
    assert G.strings() == ["AAA"] and G.unitigs["flags"].tolist() == [0] and G.edges.tolist() == [(0, 0)]
    G = hand(["ACGTACGTACGT", "TTACGTAA"], 4)
    assert G.strings() == ["GTAA", "GTAC", "TACGTA", "TTAC"]
    assert G.unitigs["nodes"].tolist() == [1, 1, 3, 1] and int(G.unitigs["kmer_count"][2]) == 10
    assert G.edges.tolist() == [(1, 2), (2, 0), (2, 1), (3, 2)]


def chain_record():
    return np.random.default_rng(11).integers(0, 4, 20000).astype(np.uint8)


def cycle_record():
    return np.tile(np.random.default_rng(7).integers(0, 4, 5000).astype(np.uint8), 3)


def pan_genome():
    rng = np.random.default_rng(3)
    g = rng.integers(0, 4, 5000).astype(np.uint8)
    out = []
    for _ in range(4):
        c = g.copy()
        at = np.nonzero(rng.random(len(c)) < 0.01)[0]
        c[at] = (c[at] + rng.integers(1, 4, len(at))) % 4
        out.append(c.astype(np.uint8))
    return out


def test_the_long_inputs():
    """the figures the GPU tests quote, from the dictionaries"""
    s = F.strings([chain_record()])
    G = CR.brute(s, 16)
    assert G.sizes() == (1, 20000, 0) and G.unitigs["nodes"].tolist() == [19985]
    G = CR.brute(s, 12)
    assert (len(G.unitigs), len(G.edges), G.counts["longest_nodes"]) == (22, 28, 4493)
    G = CR.brute(F.strings([cycle_record()]), 16)
    assert G.unitigs["nodes"].tolist() == [5000] and G.unitigs["kmer_count"].tolist() == [14985]
    assert G.unitigs["flags"].tolist() == [CR.CIRCULAR] and G.edges.tolist() == [(0, 0)]
    assert G.strings()[0][:16] == min(F.strings([cycle_record()])[0][i:i + 16] for i in range(5000))
    G = CR.brute(F.strings(pan_genome()), 21)
    assert (len(G.unitigs), len(G.edges), G.counts["nodes"]) == (487, 649, 9026)


def test_n50():
    assert CR.n50([]) == 0 and CR.n50([5]) == 5 and CR.n50([2, 2, 2, 3]) == 2 and CR.n50([10, 1, 1, 1]) == 10
