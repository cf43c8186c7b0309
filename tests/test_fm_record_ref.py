"""Definition 12 on the CPU (record_ref.py): fact 4 on every geometry case, uncapped and capped; the multi-MUMs of the
definition against a brute force over the record strings; the filter that filters nothing against repeat_ref."""
import numpy as np
import pytest

import esa_ref as ER
import fm_definition as F
import record_ref as QR
import repeat_ref as RR

CASES = F.geometry_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_fact_4_on_every_geometry_case(name):
    E = ER.of_case(name)
    for max_lcp in (0, 1, 3, 7):
        nint, _ = QR.facts(E, max_lcp)
        assert nint == len(RR.intervals(E, max_lcp)[0])
        d = QR.dup(E, max_lcp)
        assert int(d.sum()) == E.n - len(E.records)                     # every record has a row: its separator's
        if len(E.records) == 1:
            assert (QR.interval_records(E, max_lcp) == 1).all()
            assert d[0] == 0 and (d[1:] == 1).all()                     # prev[r] = r - 1: the argmin of one value


def test_fact_4_is_about_closed_ranges():
    """a range that is not closed: the formula still answers, and need not count records"""
    E = ER.of_case("dup_40x20")
    lcp, P = E.lcp(), QR.prefix(E)
    open_ranges = [(lo, hi) for lo in range(0, E.n - 3, 7) for hi in (lo + 2, lo + 3) if not QR.is_closed(lcp, lo, hi)]
    assert len(open_ranges) > 20
    assert any(QR.records(P, lo, hi) != QR.distinct(E, lo, hi) for lo, hi in open_ranges)


@pytest.mark.parametrize("k", range(6))
def test_multi_mums_against_the_record_strings(k):
    E = ER.Esa(QR.mutated_copies(11 + 100 * k))
    want = QR.brute_mums(E, min_len=1)
    rec, rc = QR.mums(E, min_len=1)
    assert (rc == 3).all() and (rec["count"] == 3).all()
    assert QR.mum_strings(E, rec) == want
    print(f"seed {11 + 100 * k}: {len(want)} multi-MUMs")
    assert len(want) >= 5
    long = {w: o for w, o in want.items() if len(w) >= 10}
    assert QR.mum_strings(E, QR.mums(E, min_len=10)[0]) == long
    # with a bound below the number of records: once in each of two or three records, nowhere else
    two, rc2 = QR.mums(E, min_len=8, min_records=2)
    assert set(rc2.tolist()) <= {2, 3} and (two["count"] == rc2).all() and len(two) >= len(QR.mums(E, min_len=8)[0])


def test_the_filter_that_filters_nothing():
    for name in ("dup_40x20", "three_identical_40_base_records", "n768"):
        E = ER.of_case(name)
        for max_lcp in (0, 7):
            for kind in RR.KINDS:
                got, rc = QR.repeats(E, kind=kind, max_lcp=max_lcp)
                assert np.array_equal(got, RR.repeats(E, kind=kind, max_lcp=max_lcp))
                assert (rc >= 1).all() and (rc <= got["count"]).all() and (rc <= len(E.records)).all()


def test_cases_with_multi_mums():
    for name in ("three_identical_40_base_records", "dup_40x20"):
        E = ER.of_case(name)
        rec, rc = QR.mums(E, min_len=1)
        assert len(rec) >= 1 and (rc == len(E.records)).all(), name
