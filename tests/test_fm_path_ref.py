"""The reference of the documented alignment (fm_path_ref.path_ref) against the references the suite already trusts, without
a GPU: its score and end cell are those of fm_chain_ref.chain_dp and of RefDP.score, its path is a valid alignment that
re-scores (RefDP.check / ChainRef.check).  Then hand-worked cases with several optimal alignments, one per clause of the
tie rule of include/debwt_hip.h, whose expected CIGAR is derived from the header in the comments."""
import numpy as np
import pytest

from conftest import golden_records
from fm_chain_ref import chain_dp
from fm_path_ref import cigar_of, path_ref
from test_fm_extend_chain_gpu import ChainRef, chains_for
from test_fm_extend_gpu import jobs_for, mutated_reads
from test_fm_search_gpu import entry_named

SCORINGS = [(1, 4, 6, 1), (2, 3, 0, 2), (1, 1, 0, 1), (255, 255, 0, 1), (255, 255, 255, 255), (1, 255, 255, 255),
            (255, 1, 0, 1), (3, 2, 1, 1)]
BANDS = [0, 1, 7, 16]


@pytest.mark.parametrize("name", ["homopolymers_tandem", "lowercase_3x2500"])
def test_reference_against_the_trusted_references(name):
    R = ChainRef(golden_records(entry_named(name)))
    total = ties = 0
    for n, w in enumerate(BANDS):
        for x in range(2):
            sc = SCORINGS[(2 * n + x + (4 if name[0] == "l" else 0)) % 8]
            rng = np.random.default_rng(31 * n + x)
            reads = mutated_reads(R, rng, 6, hi=80)
            pats, jobs = jobs_for(R, reads, rng, w)
            cpats, chains = chains_for(R, reads, rng, w)
            work = [(pats, k, s, r, [(0, d)], True) for k, s, d, r in jobs]
            work += [(cpats, k, s, r, an, False) for k, s, r, an in chains]
            for ps, k, strand, rec, an, fixed in work:
                q = R.query(ps[k], strand)
                info = {}
                got = path_ref(q, R.text, R.rs[rec], R.re[rec], an, w, sc, info)
                want, ei, et = chain_dp(q, R.text, R.rs[rec], R.re[rec], an, w, sc)
                assert got[0] == want, (ps[k], strand, rec, an, w, sc)
                if fixed:
                    assert want == R.score(ps[k], strand, an[0][1], rec, w, sc)
                if want:
                    assert info["end"] == (ei, et) == (got[2] - 1, got[4] - 1)
                R.check(ps[k], (k, strand, tuple(an), rec), w, sc, *got)
                total += 1
                ties += info["ties"] > 0
    assert total >= 200, total                              # per collection
    assert ties >= 10, ties                                 # and the rule had something to decide


def one(q, text, w, sc, diag=0):
    r = path_ref(q, text, 0, len(text), [(0, diag)], w, sc)
    return r[:6], cigar_of(r[6])


def test_end_cell_smallest_query_index_then_text_position():
    # Q = AA on T = AAAA, diag 0, w = 1: the allowed cells are (0,0) (0,1) (1,0) (1,1) (1,2).  H(0,0) = H(0,1) = a (a start;
    # E(0,1) = a - o - e is smaller), H(1,1) = H(0,0) + a = 2a and H(1,2) = H(0,1) + a = 2a.  Two cells hold the maximum in
    # row 1; the smaller text position wins: the end is (1,1), not (1,2), and the diagonal walks back to (0,0).
    for sc in SCORINGS:
        assert one("AA", "AAAA", 1, sc) == ((2 * sc[0], 0, 2, 0, 2, 0), "2M"), sc
    # Q = CA on T = AAC, w = 2: H(0,2) = 3 (C on C), H(1,0) = 3 (A on A) and H(1,1) = max(0, H(0,0) = -2) + 3 = 3.  Three
    # cells hold the maximum; the smallest query index wins although its text position is the largest: the end is (0,2).
    assert one("CA", "AAC", 2, (3, 2, 1, 1)) == ((3, 0, 1, 2, 3, 0), "1M")


def test_h_takes_the_diagonal_before_e():
    # Q = ACA on T = ACCA, (a,b,o,e) = (3,2,0,1), w = 2.  Two alignments score 3 + 3 + 3 - 1 = 8: 1M1D2M (the first C of
    # the text deleted) and 2M1D1M (the second).  Row 0: H(0,0) = 3, H(0,1) = E = H(0,0) - 1 = 2.  Row 1: H(1,1) = H(0,0) + 3
    # = 6; at (1,2) Q[1] = T[2] = C, the diagonal gives H(0,1) + 3 = 5 and E(1,2) = H(1,1) - 1 = 5: a tie.  H(2,3) =
    # H(1,2) + 3 = 8 is the end.  Walking back from (2,3): diagonal to (1,2); there the diagonal is preferred to E, so to
    # (0,1); H(0,1) came from E only: one D, opened at H(0,0), which is a start.  Hence 1M1D2M.
    assert one("ACA", "ACCA", 2, (3, 2, 0, 1)) == ((8, 0, 3, 0, 4, 1), "1M1D2M")


def test_h_takes_e_before_f():
    # Q = ACG on T = CAG, (3,2,0,1), w = 2.  Two alignments score 3 - 1 + 3 = 5 and end at (2,2): Q[1..3) = CG on CAG as
    # 1M1D1M, and ACG on T[1..3) = AG as 1M1I1M.  At (1,1) Q[1] = C, T[1] = A: the diagonal gives max(0, H(0,0) = -2) - 2 =
    # -2, E(1,1) = H(1,0) - 1 = 3 - 1 = 2 (H(1,0): C on C, a start) and F(1,1) = H(0,1) - 1 = 3 - 1 = 2 (H(0,1): A on A).
    # H(1,1) = 2 with E and F tied; H(2,2) = H(1,1) + 3 = 5.  E is preferred: the deletion of T[1], opened at H(1,0), a
    # start.  Hence 1M1D1M from query 1 and text 0.
    assert one("ACG", "CAG", 2, (3, 2, 0, 1)) == ((5, 1, 3, 0, 3, 1), "1M1D1M")


def test_a_gap_is_opened_rather_than_continued_on_a_tie():
    # Q = ACA on T = ACCGA, (3,2,0,1), w = 2: gap open 0.  2M2D1M and 1M1D1M1D1M both score 9 - 2 = 7.  Row 0: H(0,0) = 3,
    # H(0,1) = E = 2.  Row 1: H(1,1) = 6; at (1,2) the diagonal gives H(0,1) + 3 = 5 and E(1,2) = H(1,1) - 1 = 5, so
    # H(1,2) = E(1,2) = 5; at (1,3) (C on G) the diagonal gives max(0, H(0,2) = 1) - 2 = -1, F(1,3) = H(0,3) - 1 = -1 and
    # E(1,3) = max(H(1,2) - 0 - 1, E(1,2) - 1) = max(4, 4): opened and continued tie.  H(1,3) = 4 and the end is H(2,4) =
    # 7.  Walking back: diagonal to (1,3), whose H came from E; on the tie the gap is OPENED: one D and on to H(1,2), not
    # to E(1,2).  In H(1,2) the diagonal reaches 5 and is preferred, to (0,1), which is a D opened at the start (0,0).
    # Hence 1M1D1M1D1M; continuing the gap would have given 2M2D1M.
    assert one("ACA", "ACCGA", 2, (3, 2, 0, 1)) == ((7, 0, 3, 0, 5, 2), "1M1D1M1D1M")
    # the same for F: the transposed problem, T = ACA and Q = ACCGA: the walk prefers the diagonal in H(2,1) as well
    assert one("ACCGA", "ACA", 2, (3, 2, 0, 1)) == ((7, 0, 5, 0, 3, 2), "1M1I1M1I1M")


def test_stop_on_the_diagonal_where_nothing_positive_precedes():
    # Q = GAC on T = GAAC, (2,3,0,2), w = 1: H(0,0) = 2, H(0,1) = max(-3, E = H(0,0) - 2 = 0) = 0, H(1,1) = 4, and at (1,2)
    # the diagonal gives max(0, H(0,1) = 0) + 2 = 2 = E(1,2) = H(1,1) - 2.  The end cell is (1,1) (score 4, the smallest
    # row), so 2M.  With Q = TAC the best alignment is AC, ending at (2,3): in (1,2) H(0,1) = -3 <= 0, so the walk stops there.
    assert one("GAC", "GAAC", 1, (2, 3, 0, 2)) == ((4, 0, 2, 0, 2, 0), "2M")
    assert one("TAC", "GAAC", 1, (2, 3, 0, 2)) == ((4, 1, 3, 2, 4, 0), "2M")
