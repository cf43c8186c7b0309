"""The pileup reference (tests/pileup_ref.py: definitions 7 and 8 of include/debwt_hip.h) checked against its own
invariants, and the two host functions of the library, debwt_fm_ins_vote and debwt_fm_consensus, against it.  No GPU."""
import numpy as np
import pytest

import pileup_ref as R

NEW_SYMBOLS = ["debwt_fm_pileup", "debwt_fm_pile_fetch", "debwt_fm_pile_release", "debwt_fm_pile_defaults",
               "debwt_fm_pile_call", "debwt_fm_pile_insertions", "debwt_fm_ins_vote", "debwt_fm_consensus",
               "debwt_fm_pile_stats_get"]


@pytest.fixture(scope="module")
def api():
    from debwt_amd import api as A
    return A


def rand_dna(rng, n, alphabet="ACGT"):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), n))


def random_input(seed, nrec=3, naln=60):
    """record strings, reads and random valid alignments with indels (the CIGARs need not be good alignments)"""
    rng = np.random.default_rng(seed)
    strs = [rand_dna(rng, int(rng.integers(200, 400))) for _ in range(nrec)]
    text, _ = R.text_of(strs)
    n = len(text)
    pats, alns, cigars = [], [], []
    for g in range(naln):
        m = int(rng.integers(8, 120))
        pats.append(rand_dna(rng, m, "ACGTNacgt"))
        ops, q, t = [], 0, 0
        qbeg = int(rng.integers(0, 4))
        left = m - qbeg
        while left > 0:
            ln = int(rng.integers(1, min(left, 30) + 1))
            ops.append(ln << 4)
            left -= ln
            q += ln
            t += ln
            if left > 1 and rng.random() < 0.6:
                if rng.random() < 0.5:
                    k = int(rng.integers(1, min(left - 1, 4) + 1))
                    ops.append(k << 4 | 1)
                    left -= k
                else:
                    k = int(rng.integers(1, 5))
                    ops.append(k << 4 | 2)
                    t += k
        tbeg = int(rng.integers(0, n - t + 1))
        alns.append((g, tbeg, qbeg, int(rng.integers(0, 2))))
        cigars.append(ops)
    return strs, text, pats, alns, cigars


def test_abi_has_the_pileup_symbols():
    from debwt_amd import _lib
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(L, s), s


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reference_invariants(seed):
    strs, text, pats, alns, cigars = random_input(seed)
    n = len(text)
    whole = R.pileup(pats, alns, cigars, n, (0, n))
    ops = [x for c in cigars for x in c]
    mcols = sum(x >> 4 for x in ops if x & 15 == 0)
    assert sum(v for (t, s), v in whole.items() if s in (0, 1, 2, 3, 6)) == mcols
    assert sum(v for (t, s), v in whole.items() if s == 4) == sum(x >> 4 for x in ops if x & 15 == 2)
    assert sum(v for (t, s), v in whole.items() if s == 5) == sum(1 for x in ops if x & 15 == 1)
    assert not any(s == 7 for _, s in whole)
    full = R.dense(whole, (0, n))
    for win in [(0, 1), (n - 1, n), (17, 18), (100, 333), (0, n)]:
        assert R.dense(R.pileup(pats, alns, cigars, n, win), win) == full[win[0]:win[1]]
    # batches add up to the whole
    tab = {}
    for a in range(0, len(alns), 7):
        R.pileup(pats, alns[a:a + 7], cigars[a:a + 7], n, (0, n), tab)
    assert tab == whole


def test_reference_refuses_what_definition_7_refuses():
    pats, n = ["ACGTACGTAC"], 50
    ok = [(0, 5, 0, 0)]
    R.pileup(pats, ok, [[10 << 4]], n, (0, n))
    R.pileup(pats, ok, [[]], n, (0, n))
    for alns, cig, win in [(ok, [[3 << 4 | 3]], (0, n)), (ok, [[0 << 4]], (0, n)), (ok, [[1 << 4 | 1, 5 << 4]], (0, n)),
                           (ok, [[5 << 4, 1 << 4 | 2]], (0, n)), ([(1, 5, 0, 0)], [[4 << 4]], (0, n)),
                           ([(0, 5, 0, 2)], [[4 << 4]], (0, n)), ([(0, 5, 1, 0)], [[10 << 4]], (0, n)),
                           ([(0, 41, 0, 0)], [[10 << 4]], (0, n)), (ok, [[4 << 4]], (7, 7)), (ok, [[4 << 4]], (0, n + 1))]:
        with pytest.raises(R.Invalid):
            R.pileup(pats, alns, cig, n, win)


def ev_array(api, evs):
    return np.array(evs, dtype=api._INS_EVENT_DTYPE) if evs else np.zeros(0, dtype=api._INS_EVENT_DTYPE)


# reads whose query strings hold the inserted bases at known places; events are (t, aln, qpos, len)
VOTE_READS = ["AAGGTT", "aaggtt", "AACCTTN", "GGGGGG", "AANNTT"]
VOTE_ALNS = [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 1), (3, 0, 0, 0), (4, 0, 0, 0)]
VOTE_CASES = {
    "empty": [],
    "single": [(9, 0, 2, 2)],
    "case folds": [(9, 0, 2, 2), (9, 1, 2, 2), (9, 3, 0, 3)],
    "majority": [(9, 0, 2, 2), (9, 1, 2, 2), (9, 3, 0, 2), (9, 3, 1, 2), (9, 3, 2, 2)],
    "tie to the shorter": [(9, 0, 2, 2), (9, 3, 0, 1)],
    "tie to the smaller": [(9, 3, 0, 2), (9, 0, 0, 2)],
    "tie of three": [(9, 3, 0, 2), (9, 0, 2, 2), (9, 0, 0, 2), (9, 1, 0, 2), (9, 0, 4, 2), (9, 1, 4, 2)],
    "reverse strand": [(9, 2, 0, 3), (9, 2, 1, 2)],
    "non-bases are N": [(9, 4, 1, 3), (9, 4, 1, 3), (9, 0, 2, 2)],
}


@pytest.mark.parametrize("name", sorted(VOTE_CASES))
def test_ins_vote(api, name):
    evs = VOTE_CASES[name]
    want = R.vote(VOTE_READS, VOTE_ALNS, evs)
    assert api.ins_vote(VOTE_READS, VOTE_ALNS, ev_array(api, evs)) == want
    if name == "empty":
        assert want == ("", 0)
    if name == "tie to the shorter":
        assert want == ("G", 1)
    if name == "tie to the smaller":
        assert want == ("AA", 1)
    if name == "tie of three":
        assert want == ("AA", 2)
    if name == "case folds":
        assert want == ("GG", 2)
    if name == "reverse strand":
        assert R.query(VOTE_READS[2], 1) == "NAAGGTT" and want == ("AA", 1)
    if name == "non-bases are N":
        assert want == ("ANN", 2)


def test_ins_vote_refuses_events_outside_the_input(api):
    for evs in [[(9, 5, 0, 1)], [(9, 0, 5, 2)]]:
        with pytest.raises(api.DebwtError):
            api.ins_vote(VOTE_READS, VOTE_ALNS, ev_array(api, evs))


def consensus_both(api, strs, calls, window, voted, permille=600):
    text, starts = R.text_of(strs)
    want = R.consensus(text, starts, calls, window, voted, permille)
    ref = [R.SLOT.get(c, 4) for c in text[window[0]:window[1]]]
    ins = [(t, s, sup, d) for t, (s, sup, d) in voted.items()]
    got = api.consensus(ref, calls, window, ins, starts, len(text), permille)
    assert got == want
    return got


def test_consensus_cases(api):
    strs = ["ACGTACGTAC", "G", "TTTTGGGG"]
    text, starts = R.text_of(strs)
    n = len(text)
    ident = [R.SLOT.get(c, R.NO_CALL) for c in text]
    assert consensus_both(api, strs, ident, (0, n), {}) == strs
    # a no-call run, a substitution, a deletion next to an insertion, and the record of one base
    calls = list(ident)
    calls[2:5] = [R.NO_CALL] * 3
    calls[6] = 0
    calls[7] = R.DEL
    calls[8] = ident[8] | R.INS_BIT
    calls[11] = 1 | R.INS_BIT
    voted = {8: ("TT", 3, 4), 11: ("ACG", 4, 4)}
    got = consensus_both(api, strs, calls, (0, n), voted)
    assert got == ["ACgtaCAATTC", "CACG", "TTTTGGGG"]
    # an insertion flagged without a voted string, and one whose support misses the line: 2 of 4 at 600, on it at 500
    assert consensus_both(api, strs, calls, (0, n), {11: ("ACG", 2, 4)})[:2] == ["ACgtaCAAC", "C"]
    assert consensus_both(api, strs, calls, (0, n), {11: ("ACG", 2, 4)}, 500)[1] == "CACG"
    # windows: inside one record, across a separator, one position, the separator alone
    for win in [(3, 9), (8, 14), (11, 12), (10, 11), (12, n)]:
        consensus_both(api, strs, calls[win[0]:win[1]], win, voted)
    assert consensus_both(api, strs, calls[10:11], (10, 11), {}) == ["", "", ""]


def test_call_reference_tie_rules():
    text = "ACGT#A$"
    def one(t, c, **kw):
        counts = {(t, s): v for s, v in enumerate(c) if v}
        calls, refs, var = R.call(counts, text, (t, t + 1), **kw)
        return calls[0], var
    assert one(1, [2, 2, 0, 0, 0]) == (R.NO_CALL, [])                    # 2 of 4 is below 600
    assert one(1, [2, 2, 0, 0, 0], min_permille=500) == (1, [])          # tie: the reference base wins
    assert one(2, [3, 3, 0, 0, 0], min_permille=500)[0] == 0             # tie without the reference: the lowest
    assert one(1, [0, 3, 0, 0, 0]) == (R.NO_CALL, [])                    # depth 3 < 4
    assert one(1, [0, 0, 0, 0, 4]) == (4, [(1, 4, 4, 0, 1, 4)])          # a called deletion
    assert one(4, [9, 0, 0, 0, 0]) == (R.NO_CALL, [])                    # a separator is never called
    assert one(1, [0, 3, 0, 2, 0]) == (1, [])                            # 3 of 5 is exactly 600
    assert one(1, [0, 5, 0, 0, 0, 3]) == (1 | R.INS_BIT, [(1, 5, 5, 3, 1, 1 | R.INS_BIT)])
    assert one(1, [0, 5, 0, 0, 0, 2]) == (1, [])
    assert one(1, [0, 2, 0, 0, 0, 9, 50]) == (R.NO_CALL, [])             # slot 6 is no depth; no bit without a call
