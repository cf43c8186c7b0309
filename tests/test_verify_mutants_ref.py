"""The mutant sweep of the inverse-BWT verifiers on the CPU (tests/verify_mutants.py): the plain reference accepts the
definition's rows of every case and rejects every mutant, the classes are what they claim to be and none is empty, the
restated boundary placement gives several segments, and the host tool debwt_verify_inverse rejects every mutant that the
reference rejects -- exhaustively, every class on every case."""
import collections

import numpy as np
import pytest

import fm_definition as F
import verify_mutants as M

every_case = pytest.mark.parametrize("name", M.CASE_NAMES)


def test_the_new_cases_are_what_they_are_for():
    for name in M.CASE_NAMES:
        D = M.case(name)
        assert min(len(r) for r in D.records) > 32 and D.n > D.nrec * 32, name      # the loader takes them
        assert 383 <= D.n <= 1152
    D = M.case("all_T_400_37_33")
    assert [len(r) for r in D.records] == [400, 37, 33] and D.census().tolist() == [0, 0, 0, D.n]
    assert int(np.count_nonzero(D.L < 3)) == 0                                      # C['T'] = 0
    D = M.case("recs_30x33")
    assert D.nrec == 30 and D.n == 1020 and D.n - D.nrec * 32 == 60
    D = M.case("no_T_200_150_100")
    assert int(D.census()[3]) == D.nrec == 3 and not (D.sym == 3).any()


@every_case
def test_reference_accepts_the_definition_rows_and_rejects_every_mutant(name):
    D = M.case(name)
    assert M.reference_verdict(D.words, D.n, D.hash_rows, D.dollar_row, D.sym) == (True, None)
    good = (M.codes_of(D.words, D.n).tobytes(), D.hash_rows.tobytes(), D.dollar_row)
    for i, (cls, words, hrows, drow) in enumerate(M.mutant_list(name)):
        v = M.reference_verdict(words, D.n, hrows, drow, D.sym)
        same = (M.codes_of(words, D.n).tobytes(), hrows.tobytes(), drow) == good
        if cls == "P":
            assert same and not np.array_equal(words, D.words) and v == (True, None), (cls, i)
            continue
        assert not v.accepted, (cls, i, drow)
        assert not same, (cls, i)
        if cls in ("E", "F"):
            assert v.refused, (cls, i)
        elif cls not in ("C3", "D"):
            assert v.refused is None, (cls, i, v)               # a well-formed triple that is not the text's BWT
        if cls.startswith("B") or cls.startswith("C"):
            assert np.array_equal(np.bincount(M.codes_of(words, D.n), minlength=4), D.census()), (cls, i)
        if cls in ("C1", "C2", "C3", "D", "F"):
            assert words is D.words


@every_case
def test_the_guards_decide_c3_and_d(name):
    """verify_mutants.guard_applies, which tells the GPU tests whether to expect DEBWT_EINVAL or a failed walk, against
    the reference on every mutant: a C3 or D mutant is a refused input exactly when its moved row holds no code 3 or is
    a listed row of the other kind; both kinds occur"""
    D = M.case(name)
    seen = set()
    for cls, words, hrows, drow in M.mutant_list(name):
        if cls == "P":
            continue
        v = M.reference_verdict(words, D.n, hrows, drow, D.sym)
        assert bool(v.refused) == M.guard_applies(D, cls, words, hrows, drow), (cls, drow, v)
        seen.add((cls, bool(v.refused)))
    assert ("D", True) in seen and (("D", False) in seen or name == "no_T_200_150_100")


def test_every_class_is_populated():
    count = {name: collections.Counter(m[0] for m in M.mutant_list(name)) for name in M.CASE_NAMES}
    for cls in M.CLASSES:
        assert sum(1 for name in M.CASE_NAMES if count[name][cls]) >= 3, cls
    for name in ("all_T_400_37_33", "recs_30x33"):
        assert count[name]["C1"], name
    for name in M.CASE_NAMES:                                   # complete where nothing stands in the way
        D = M.case(name)
        assert count[name]["A"] == 3 * (D.n - D.nrec) and count[name]["D"] == D.n - 1 and count[name]["E"] == 3 * D.nrec
        assert count[name]["C2"] == D.nrec - 1 and count[name]["F"] == (9 if D.nrec > 2 else 6 if D.nrec == 2 else 3)
    assert max(sum(c.values()) for c in count.values()) < 10_000


@every_case
def test_reference_rejects_the_rows_on_every_mutated_text(name):
    D = M.case(name)
    seen = 0
    for cls, recs in M.text_mutants(D.records):
        sym = F.text_symbols(recs)
        assert len(sym) == D.n and len(recs) == D.nrec and min(len(r) for r in recs) > 32
        assert not np.array_equal(sym, D.sym)
        assert not M.reference_verdict(D.words, D.n, D.hash_rows, D.dollar_row, sym).accepted
        seen += 1
    swaps = sum((len(a) > 33) + (len(b) > 33) for a, b in zip(D.records, D.records[1:]))
    assert seen == D.n - D.nrec + swaps


ONE_SEGMENT = ("dup_40x20", "all_T_400_37_33")                 # equal records / one letter: no context is unique
SHORT_CONTEXT_AT_64 = ("n383", "n384", "n385", "no_T_200_150_100")


@every_case
def test_expected_segments(name):
    """The GPU tests want walks cut into several segments, so that the links between segments are under test: at least 4
    at segments = 64 on every case but the two of ONE_SEGMENT.  That holds from n = 753 up (33 to 64 segments).  On the
    four cases of SHORT_CONTEXT_AT_64 it cannot: n // 64 gives gap = 5 to 7 and the library's maxm = gap // 2 is 2 or 3
    symbols, and at most 4^3 = 64 base contexts cannot be unique among 383 and more positions (1, 1, 1 and 2 segments:
    only a context next to a separator is).  Those cases get their segments at segments = 7: gap = 54 to 64, maxm = 27
    to 32, every boundary found, 7 or 8 segments -- asserted here for all nine cases."""
    D = M.case(name)
    seg = {s: M.expected_segments(D.sym, D.sa, D.n, s) for s in (0, 1, 7, 64)}
    assert seg[0] == seg[1] == 1
    for segments in (7, 64):
        b = M.expected_bounds(D.sym, D.sa, D.n, segments)
        assert all(0 < p < D.n - 1 and int(D.sa[r]) == p for p, r in b)
        assert [p for p, _ in b] == sorted({p for p, _ in b})
        assert seg[segments] <= segments + 1
    if name in ONE_SEGMENT:
        assert seg[7] == seg[64] == 1
        return
    assert seg[7] == (D.n - 2) // (D.n // 7) + 1 and seg[7] in (7, 8)      # every boundary found
    if name in SHORT_CONTEXT_AT_64:
        assert (D.n // 64) // 2 <= 3 and seg[64] <= 2
    else:
        assert seg[64] >= 4


@every_case
def test_the_segmented_walk_refuses_what_the_reference_refuses(name):
    """verify_mutants.segmented_report, the device verifier's counters restated (the GPU tests compare a sample of the
    device's reports with it): a clean report with the expected segments on the true rows at every setting, and on every
    well-formed mutant, at one of the four settings in turn, counters that do not add up to an accepted walk.

    A verifier that left broken_links out of its verdict would still refuse every one of them: no mutant here, and
    none of 1.2 million random changes of one to four rows tried at segments 7 and 64 while this was written, is refused
    by a broken link alone.  A boundary's row is the only row whose suffix starts with the boundary's context, by the
    rows' own counts, and a walk that has spelled that context without a mismatch ends on a row whose suffix starts
    with it; so a link breaks only after a symbol somewhere else has."""
    D = M.case(name)
    for segments in (0, 1, 7, 64):
        rep = M.segmented_report(D.words, D.n, D.hash_rows, D.dollar_row, D.sym, segments)
        assert M.report_accepts(rep, D.n) and rep["segments"] == M.expected_segments(D.sym, D.sa, D.n, segments), rep
    links = 0
    for i, (cls, words, hrows, drow) in enumerate(M.mutant_list(name)):
        if M.guard_applies(D, cls, words, hrows, drow):
            continue
        rep = M.segmented_report(words, D.n, hrows, drow, D.sym, (0, 1, 7, 64)[i % 4])
        assert M.report_accepts(rep, D.n) == (cls == "P"), (cls, i, rep)
        links += rep["broken_links"] > 0
        assert rep["mismatches"] or rep["search_failures"] or cls == "P", (cls, i, rep)
    assert links or name in ONE_SEGMENT + SHORT_CONTEXT_AT_64 + ("n1152_single",), links


# ---- the host tool on every mutant -------------------------------------------------------------------------------------

@every_case
def test_host_tool_rejects_every_mutant(name):
    """debwt_verify_inverse: A to E are rejected, by a nonzero code or by a decoded text that is not the text; F gets a
    nonzero code; P changes nothing.  Where the reference names a format refusal the code is DEBWT_EINVAL (-1)."""
    from debwt_amd import api
    D = M.case(name)
    rc, inv = api.verify_inverse(D.words, D.n, D.hash_rows, D.dollar_row)
    assert rc == 0 and np.array_equal(inv, D.sym)
    for i, (cls, words, hrows, drow) in enumerate(M.mutant_list(name)):
        rc, inv = api.verify_inverse(words, D.n, hrows, drow)
        if cls == "P":
            assert rc == 0 and np.array_equal(inv, D.sym), (cls, i)
        elif cls == "F":
            assert rc != 0, (cls, i)
        else:
            assert rc != 0 or not np.array_equal(inv, D.sym), (cls, i, drow)
        if cls != "P" and M.reference_verdict(words, D.n, hrows, drow, D.sym).refused:
            assert rc == -1, (cls, i, rc)
    rc, inv = api.verify_inverse(D.words, D.n, D.hash_rows, D.dollar_row)
    assert rc == 0 and np.array_equal(inv, D.sym)
