"""Definition 14 on the CPU (bicdbg_ref.py): the dictionary brute force against the interval rules over esa_ref.Esa on
every geometry case (both assert the mirror properties and facts 1 to 3), Definition 13 on the doubled collection folded
as the second witness wherever there is no hairpin, the hand examples of the definition, and the inputs the GPU tests rest
on with the figures the definition gives for them."""
import numpy as np
import pytest

import bicdbg_ref as BR
import cdbg_ref as CR
import esa_ref as ER
import fm_definition as F
from test_fm_cdbg_ref import chain_record, codes, cycle_record, pan_genome

CASES = F.geometry_cases()
KS = (1, 3, 5, 7)


def both_ways(strs, k, E=None):
    E = E or ER.Esa(codes(strs))
    G = BR.from_esa(E, k)
    B = BR.brute(strs, k)
    BR.same_graph(G, B, rows=False)
    assert G.strings() == B.strings()
    return G


def folds(strs, k, G):
    """Definition 13 on the doubled collection, folded, against G"""
    D = F.strings(BR.doubled(codes(strs)))
    assert BR.fold(CR.brute(D, k), k, BR.kmers_of(strs, k)) == BR.folded(G)


@pytest.mark.parametrize("name", list(CASES))
def test_geometry_cases(name):
    E = ER.of_case(name)
    strs = F.strings(CASES[name])
    for k in KS:
        G = both_ways(strs, k, E)
        BR.same_graph(G, BR.from_esa(E, k, max_lcp=k + 1))
        for s, u in zip(G.strings(), G.unitigs):                    # row_lo is the first row of w*, a k-mer of the unitig
            w = "".join(F.ACGT[c] for c in E.sym[int(E.sa[int(u["row_lo"])]):][:k].tolist())
            assert w in s and (not u["flags"] or s.startswith(w))


def test_the_doubled_collection_folds_to_the_same_answer():
    done = total = 0
    for name in CASES:
        strs = F.strings(CASES[name])
        if sum(len(s) for s in strs) > 1500:
            continue
        for k in KS:
            G = BR.brute(strs, k)
            total += 1
            if G.counts["hairpins"] == 0:
                folds(strs, k, G)
                done += 1
    print(f"{done} of {total} cases have no hairpin")
    assert 2 * done >= total


def test_hairpin():
    G = both_ways(["ACGT"], 3)                                      # ACG and CGT are mirrors: the edge ACGT joins them
    assert G.counts["hairpins"] == 1 and G.strings() == ["ACG"] and G.edges.tolist() == [(0, 1)]
    assert G.unitigs["kmer_count"].tolist() == [2] and G.counts["mated"] == 2
    G = both_ways(["TTACGTCC"], 3)
    assert G.counts["hairpins"] >= 1 and "ACGT" not in "".join(G.strings()) + "|" + "|".join(F.revcomp(s) for s in G.strings())
    G = both_ways(["ACGTACGTACGT"], 3)                              # ACG > CGT > GTA > TAC > ACG, its own mirror image
    assert G.counts["present"] == 4 and G.counts["mated"] == 4 and G.counts["nodes"] == 2
    assert G.counts["hairpins"] == 2 and G.strings() == ["TACG"]    # TAC > ACG is a link, and so is its mirror CGT > GTA
    assert G.edges.tolist() == [(0, 1), (1, 0)]                     # ACGT joins the unitig's end to its mirror, GTAC back
    assert G.unitigs["kmer_count"].tolist() == [10] and G.unitigs["flags"].tolist() == [0]


def canonical(G):
    """the answer without its choice of orientation and numbering: unitigs by the lower of string and reverse complement,
    edges between (that string, orientation relative to it)"""
    strs = G.strings()
    low = [min(s, F.revcomp(s)) for s in strs]
    un = sorted((low[i], int(u["nodes"]), int(u["kmer_count"]), int(u["flags"])) for i, u in enumerate(G.unitigs))
    end = lambda x: (low[x >> 1], (x & 1) ^ (strs[x >> 1] != low[x >> 1]))                    # noqa: E731
    return un, sorted((end(int(e["from"])), end(int(e["to"]))) for e in G.edges)


def test_record_with_its_reverse_complement():
    """Every node is mated, and the answer is that of the record alone with kmer_count doubled.  The reported orientation
    and the numbering may differ: w* is the lowest k-mer that OCCURS, and more occur now."""
    s = F.strings([np.random.default_rng(5).integers(0, 4, 300).astype(np.uint8)])[0] + "ACCA"
    for k in (3, 5, 7, 11):
        one, two = both_ways([s], k), both_ways([s, F.revcomp(s)], k)
        assert two.counts["mated"] == two.counts["present"] and one.counts["mated"] < one.counts["present"]
        assert one.counts["circular"] == 0
        (u1, e1), (u2, e2) = canonical(one), canonical(two)
        assert e1 == e2 and [(a, b, 2 * c, d) for a, b, c, d in u1] == u2
        assert {x: one.counts[x] for x in CR.COUNTING} == {x: two.counts[x] for x in CR.COUNTING}
        assert one.strings() != two.strings() or k == 11


def test_edge_string_with_its_reverse_complement():
    """both collections hold an edge string together with its reverse complement: one pair in the list, not two"""
    for strs, k in ((["AACCGTT", "AACGGTT"], 3), (["ACCAGT", "ACTGGT", "CCAGA"], 3)):
        es = {s[i:i + k + 1] for s in strs for i in range(len(s) - k)}
        assert any(F.revcomp(e) in es and F.revcomp(e) != e for e in es)
        G = both_ways(strs, k)
        assert len(set(map(tuple, G.edges.tolist()))) == len(G.edges)
        if G.counts["hairpins"] == 0:
            folds(strs, k, G)


def test_the_long_inputs():
    """the figures the GPU tests quote, from the dictionaries"""
    s = F.strings([chain_record()])
    G = BR.brute(s, 15)
    assert G.sizes() == (1, 20000, 0) and G.unitigs["nodes"].tolist() == [19986] and G.counts["mated"] == 0
    cyc = F.strings([cycle_record()])[0]
    low = min(cyc[i:i + 15] for i in range(5000))
    for strs in ([cyc], [cyc, F.revcomp(cyc)]):
        G = BR.brute(strs, 15)
        assert G.unitigs["nodes"].tolist() == [5000] and G.unitigs["kmer_count"].tolist() == [14986 * len(strs)]
        assert G.unitigs["flags"].tolist() == [CR.CIRCULAR] and G.edges.tolist() == [(0, 0), (1, 1)]
        assert G.counts["circular"] == 1 and G.counts["mated"] == (0 if len(strs) == 1 else 10000)
        w = G.strings()[0][:15]
        assert w == (low if len(strs) == 1 else min(low, min(F.revcomp(cyc)[i:i + 15] for i in range(5000))))
    pan = F.strings(pan_genome())
    G = BR.brute(pan, 21)
    assert G.counts["hairpins"] == 0
    assert (len(G.unitigs), len(G.edges), G.counts["nodes"]) == PAN_21
    folds(pan, 21, G)


PAN_21 = (487, 1298, 9026)
# the k of 15, 21, 31 at which the answer has no hairpin, so that the doubled index is a witness on the GPU
FOLD_READS, FOLD_PAN = (21, 31), (15, 21, 31)


def mixed_reads():
    """the seeded read set with every second read reverse-complemented"""
    recs = ER.of_read_set().records
    return [BR.rc_codes(r) if i & 1 else r for i, r in enumerate(recs)]


def test_which_k_have_no_hairpin():
    E = ER.Esa(mixed_reads())
    pan = F.strings(pan_genome())
    seen = {}
    for k in (15, 21, 31):
        G = BR.from_esa(E, k)
        seen[k] = (G.counts["hairpins"], G.counts["unitigs"], G.counts["edges"], G.counts["mated"], G.counts["present"])
        assert (G.counts["hairpins"] == 0) == (k in FOLD_READS)
        assert (BR.brute(pan, k).counts["hairpins"] == 0) == (k in FOLD_PAN)
    assert seen == {15: (1, 1811, 4455, 6318, 16088), 21: (0, 1640, 3804, 6330, 18237), 31: (0, 1338, 2642, 6244, 19492)}
