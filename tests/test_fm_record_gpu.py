"""Distinct records per LCP interval on the GPU (debwt_fm_records_build and what stands on it; EsaResult.records_build,
dup_prefix, record_counts, repeats_by_record, mums) against Definition 12 as record_ref.py writes it out.  Everything is
compared exactly: every geometry case at fanout 64 and at fanout 2, pairs whose rows lie far apart with the bound that pins
the logarithmic range minimum, the staircase of a homopolymer, the seeded read set (a two-pass sort), a capped build, and
the protocol."""
import ctypes

import numpy as np
import pytest

import esa_ref as ER
import fm_definition as F
import record_ref as QR
import repeat_ref as RR
from test_fm_esa_gpu import index_of

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, ERANGE = -1, -4, -5
CASES = F.geometry_cases()
FILTERS = ({}, {"unique": True}, {"min_records": 2}, {"max_records": 1})


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


@pytest.fixture(autouse=True)
def default_limits(monkeypatch):
    monkeypatch.delenv("DEBWT_FM_REPEAT_FANOUT", raising=False)
    monkeypatch.delenv("DEBWT_FM_ESA_CHUNK", raising=False)


def levels_of(n, fanout):
    t = 0
    while n > 1:
        n, t = -(-n // fanout), t + 1
    return t


def bits_of(v):
    return int(v).bit_length()


def check_build(x, e, E, fanout, max_lcp=0):
    """the prefix array and the statistics of the build"""
    e.records_build()
    P = e.dup_prefix()
    assert P.dtype == np.uint64 and np.array_equal(P, QR.prefix(E, max_lcp))
    st = x.records_stats()
    nrec = len(E.records)
    assert st["rows"] == E.n and st["pairs"] == E.n - nrec and st["records_present"] == nrec
    assert st["fanout"] == fanout and st["levels"] == levels_of(E.n, fanout)
    assert st["sort_passes"] == -(-bits_of(nrec - 1) // 8) and st["kept_bytes"] == 8 * E.n < st["build_bytes"]
    assert st["rmq_steps"] <= st["pairs"] * 3 * fanout * (st["levels"] + 1) and st["rmq_steps"] <= st["wave_steps"]
    assert (st["rmq_steps"] > 0) == (st["pairs"] > 0)
    return st


def check_filters(e, E, max_lcp=0, min_len=1):
    for kind in RR.KINDS:
        for flt in FILTERS:
            want, wrc = QR.repeats(E, min_len=min_len, kind=kind, max_lcp=max_lcp, **flt)
            got, rc = e.repeats_by_record(min_len=min_len, kind=kind, **flt)
            assert got.dtype == RR.DTYPE and rc.dtype == np.uint32
            assert np.array_equal(got, want) and np.array_equal(rc, wrc), (kind, flt)
        plain = e.repeats(min_len=min_len, kind=kind)                       # the filter {1, 0, 0}: byte for byte
        assert e.repeats_by_record(min_len=min_len, kind=kind)[0].tobytes() == plain.tobytes()


def seeded_patterns(E, rng, count, cap=None):
    """strings taken from the rows (so they occur), cut to at most cap bases, and a few that need not occur"""
    out = []
    for r in rng.integers(0, E.n, count).tolist():
        top = int(E.d[r]) if cap is None else min(int(E.d[r]), cap)
        if top >= 1:
            k = int(rng.integers(1, min(top, 40) + 1))
            out.append("".join(F.ACGT[c] for c in E.sym[int(E.sa[r]):int(E.sa[r]) + k]))
    out += ["".join(F.ACGT[c] for c in rng.integers(0, 4, 6)) for _ in range(8)]
    return out


def check_counts(x, e, E, rng, max_lcp=0):
    """record_counts on every interval, and on the ranges count answers for seeded patterns"""
    every = RR.intervals(E, max_lcp)[0]
    if len(every):
        rg = np.stack([every["row_lo"], every["row_lo"] + every["count"]], axis=1)
        assert np.array_equal(e.record_counts(rg), QR.interval_records(E, max_lcp))
    pats = seeded_patterns(E, rng, 40, max_lcp or None)
    rg = x.ranges(pats)
    got = e.record_counts(rg)
    assert got.dtype == np.uint64
    assert got.tolist() == [QR.distinct(E, lo, hi) for lo, hi in rg.tolist()]
    assert len(e.record_counts(np.zeros((0, 2), dtype=np.uint64))) == 0


# ---- every geometry case ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fanout", [64, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_geometry_cases(api, monkeypatch, name, fanout):
    E = ER.of_case(name)
    monkeypatch.setenv("DEBWT_FM_REPEAT_FANOUT", str(fanout))
    x = index_of(api, CASES[name], 32)
    e = x.esa(sa=True, da=True)
    check_build(x, e, E, fanout)
    check_filters(e, E)
    check_counts(x, e, E, np.random.default_rng(len(name) + fanout))
    every, rc = e.repeats_by_record(min_len=1, kind="intervals")
    if len(E.records) == 1:
        assert (rc == 1).all() and len(e.mums(min_len=1)[0]) == 0
    if name in ("three_identical_40_base_records", "dup_40x20"):
        got, grc = e.mums(min_len=1)
        want, wrc = QR.mums(E, min_len=1)
        assert len(got) >= 1 and np.array_equal(got, want) and np.array_equal(grc, wrc) and (grc == len(E.records)).all()
    if name == "ones_600":                                                  # the atomics pile up on a few rows
        assert int(QR.dup(E).max()) > 100
    x.close()


# ---- the bound that pins the logarithmic range minimum ------------------------------------------------------------------

def long_pairs():
    rng = np.random.default_rng(2027)
    return [rng.integers(0, 4, 20000).astype(np.uint8), rng.integers(0, 4, 60).astype(np.uint8)]


@pytest.mark.parametrize("fanout", [64, 2])
def test_long_pairs(api, monkeypatch, fanout):
    """Two records, 20,000 and 60 random bases: neighbouring rows of the short record lie hundreds of rows apart, so the
    range minimum crosses levels.  A pair costs at most 2 (F - 1) reads per level going up and F per level going down."""
    E = ER.Esa(long_pairs())
    gaps = np.diff(np.nonzero(E.da == 1)[0])
    assert len(gaps) == 60 and int(np.median(gaps)) > 100
    monkeypatch.setenv("DEBWT_FM_REPEAT_FANOUT", str(fanout))
    x = index_of(api, E.records, 32)
    e = x.esa(da=True)
    st = check_build(x, e, E, fanout)
    bound = st["pairs"] * 3 * fanout * (st["levels"] + 1)
    print(f"fanout {fanout}: rmq_steps {st['rmq_steps']}, bound {bound}, wave_steps {st['wave_steps']}, levels {st['levels']}")
    assert 0 < st["rmq_steps"] <= bound and st["rmq_steps"] <= st["wave_steps"]
    check_filters(e, E, min_len=6)
    x.close()


def test_homopolymer_staircase(api):
    """One record of 20,000 'T': prev[r] = r - 1, so dup[r] = 1 for every r >= 1"""
    E = ER.of_homopolymer(20000)
    x = index_of(api, E.records, 32)
    e = x.esa(da=True)
    e.records_build()
    assert np.array_equal(e.dup_prefix(), np.arange(E.n, dtype=np.uint64))
    st = x.records_stats()
    assert st["pairs"] == E.n - 1 and st["records_present"] == 1 and st["sort_passes"] == 0
    every, rc = e.repeats_by_record(min_len=1, kind="intervals")
    assert len(every) == 19999 and (rc == 1).all()
    assert len(e.repeats_by_record(min_len=1, kind="intervals", min_records=2)[0]) == 0
    x.close()


# ---- the seeded read set ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fm(api):
    x = index_of(api, ER.of_read_set().records, 4)
    yield x
    x.close()


@pytest.mark.parametrize("fanout", [64, 8])
def test_read_set(api, fm, monkeypatch, fanout):
    E = ER.of_read_set()
    assert E.n == 104715 and len(E.records) == 1581
    monkeypatch.setenv("DEBWT_FM_REPEAT_FANOUT", str(fanout))
    e = fm.esa(sa=True, da=True)
    st = check_build(fm, e, E, fanout)
    assert st["sort_passes"] == 2 and st["pairs"] == E.n - 1581
    for kind, flt in (("intervals", {"min_records": 8}), ("maximal", {"unique": True}), ("intervals", {"max_records": 3}),
                      ("maximal", {"min_records": 4, "max_records": 12, "unique": True})):
        want, wrc = QR.repeats(E, min_len=20, kind=kind, **flt)
        got, rc = e.repeats_by_record(min_len=20, kind=kind, **flt)
        assert len(want) > 0 and np.array_equal(got, want) and np.array_equal(rc, wrc), (kind, flt)
        assert fm.repeat_stats()["reported"] == len(want)
    assert len(QR.repeats(E, min_len=20, kind="intervals", min_records=8)[0]) == 17587
    assert len(QR.repeats(E, min_len=20, kind="maximal", unique=True)[0]) == 11587
    assert e.repeats_by_record(min_len=20)[0].tobytes() == e.repeats(min_len=20).tobytes()
    check_counts(fm, e, E, np.random.default_rng(fanout))
    e.release()


# ---- a capped build -----------------------------------------------------------------------------------------------------

def test_capped_build(api, fm):
    E, max_lcp = ER.of_read_set(), 7
    e = fm.esa(max_lcp=max_lcp, da=True)
    check_build(fm, e, E, 64, max_lcp)
    for kind, flt in (("intervals", {}), ("intervals", {"min_records": 8}), ("maximal", {"unique": True})):
        want, wrc = QR.repeats(E, kind=kind, max_lcp=max_lcp, **flt)
        got, rc = e.repeats_by_record(min_len=1, kind=kind, **flt)
        assert len(want) > 0 and int(want["len"].max()) < max_lcp
        assert np.array_equal(got, want) and np.array_equal(rc, wrc), (kind, flt)
    check_counts(fm, e, E, np.random.default_rng(7), max_lcp)
    # ranges that are not closed: still the value of the formula, whatever it counts
    rng = np.random.default_rng(77)
    lo = rng.integers(0, E.n - 400, 300)
    rg = np.stack([lo, lo + rng.integers(0, 400, 300)], axis=1).astype(np.uint64)
    lcp, P = E.lcp(max_lcp), QR.prefix(E, max_lcp)
    assert sum(not QR.is_closed(lcp, int(a), int(b)) for a, b in rg.tolist()) > 100
    assert np.array_equal(e.record_counts(rg), QR.records_of(P, rg))
    e.release()


# ---- protocol -----------------------------------------------------------------------------------------------------------

def code_of(api, fn, *args, **kw):
    with pytest.raises(api.DebwtError) as err:
        fn(*args, **kw)
    return err.value.code


def raw(x, opts, flt, out, recs, capacity, count=True):
    from debwt_amd import _lib
    n = ctypes.c_uint64(12345)
    o = None if opts is None else ctypes.byref(_lib.DebwtFmRepeatOpts(*opts))
    f = None if flt is None else ctypes.byref(_lib.DebwtFmRecordFilter(*flt))
    p = None if out is None else out.ctypes.data_as(ctypes.c_void_p)
    q = None if recs is None else recs.ctypes.data_as(ctypes.c_void_p)
    rc = x._L.debwt_fm_repeats_records(x._h, o, f, p, q, capacity, ctypes.byref(n) if count else None)
    return rc, n.value


def test_protocol(api):
    name = "dup_40x20"
    E = ER.of_case(name)
    x = index_of(api, CASES[name], 4)
    ok, all_ = (1, 2, 2, 0), (1, 0, 0, 0)
    before = api.EsaResult(x)
    assert code_of(api, before.records_build) == ESTATE                     # no build
    b_none = x.info()["device_bytes"]
    e = x.esa(sa=True)                                                      # a build without da
    assert code_of(api, e.records_build) == ESTATE
    e = x.esa(da=True)
    assert code_of(api, e.dup_prefix) == ESTATE                             # da, but no records build
    assert code_of(api, e.record_counts, [[0, 1]]) == ESTATE
    assert code_of(api, e.repeats_by_record, min_len=1) == ESTATE and raw(x, ok, all_, None, None, 0) == (ESTATE, 12345)
    assert len(e.repeats(min_len=1)) > 0                                    # debwt_fm_repeats needs none

    b0 = x.info()["device_bytes"]
    e.records_build()
    st = x.records_stats()
    assert st["kept_bytes"] == 8 * E.n and x.info()["device_bytes"] == b0 + st["kept_bytes"]
    P = e.dup_prefix()
    e.records_build()                                                       # a second build replaces the first
    assert x.info()["device_bytes"] == b0 + st["kept_bytes"] and np.array_equal(e.dup_prefix(), P)
    assert np.array_equal(e.dup_prefix(5, 30), P[5:30]) and len(e.dup_prefix(E.n, E.n)) == 0
    assert code_of(api, e.dup_prefix, 1, E.n + 1) == EINVAL

    assert code_of(api, e.record_counts, [[0, E.n + 1]]) == EINVAL          # hi > n
    assert code_of(api, e.record_counts, [[0, 3], [5, 4]]) == EINVAL        # lo > hi
    assert e.record_counts([[0, E.n], [3, 3], [E.n, E.n]]).tolist() == [len(E.records), 0, 0]

    want, wrc = QR.repeats(E, min_len=1, kind="intervals")
    count = len(want)
    assert count > 10
    buf, rbuf = np.zeros(count + 1, dtype=RR.DTYPE), np.zeros(count + 1, dtype=np.uint32)
    assert raw(x, ok, None, None, None, 0) == (EINVAL, 12345)               # no filter
    assert raw(x, None, all_, None, None, 0)[0] == EINVAL and raw(x, ok, all_, None, None, 0, count=False)[0] == EINVAL
    for bad in ((0, 0, 0, 0), (3, 2, 0, 0), (1, 0, 2, 0), (1, 0, 0x80000000, 0), (1, 0, 0, 1)):
        assert raw(x, ok, bad, None, None, 0) == (EINVAL, 12345), bad
    for bad in ((0, 2, 2, 0), (1, 2, 1, 0), (1, 2, 5, 4), (1, 3, 2, 0)):    # the errors of debwt_fm_repeats
        assert raw(x, bad, all_, None, None, 0) == (EINVAL, 12345), bad
    assert raw(x, ok, all_, None, None, 1)[0] == EINVAL                     # no out with capacity > 0
    assert raw(x, ok, (2, 2, 0, 0), None, None, 0)[0] in (0, ERANGE)        # max_records == min_records is a filter
    assert raw(x, ok, all_, None, None, 0) == (ERANGE, count)               # the sizing call
    assert raw(x, ok, all_, buf, rbuf, count - 1) == (ERANGE, count) and not buf.view(np.uint8).any() and not rbuf.any()
    assert raw(x, ok, all_, buf, rbuf, count) == (0, count)
    assert np.array_equal(buf[:count], want) and np.array_equal(rbuf[:count], wrc)
    assert not buf[count:].view(np.uint8).any() and not rbuf[count:].any()
    buf[:] = 0
    assert raw(x, ok, all_, buf, None, count + 1) == (0, count) and np.array_equal(buf[:count], want)   # no records array
    assert raw(x, ok, (10 ** 6, 0, 0, 0), None, None, 0) == (0, 0)          # no interval in that many records
    assert x.repeat_stats()["reported"] == 0 and x.repeat_stats()["intervals"] == count
    with pytest.raises(ValueError):
        e.repeats_by_record(kind="tandem")

    from debwt_amd import _lib
    four = np.zeros(4, dtype=np.uint32)
    assert x._L.debwt_fm_esa_fetch(x._h, 3, 0, 4, four.ctypes.data_as(ctypes.c_void_p)) == EINVAL   # the prefix is no fourth array

    e = x.esa(max_lcp=5, da=True)                                           # the next esa build releases the prefix
    assert x.info()["device_bytes"] == b0 and code_of(api, e.dup_prefix) == ESTATE
    e.records_build()
    assert np.array_equal(e.dup_prefix(), QR.prefix(E, 5))
    e.release()
    assert x.info()["device_bytes"] == b0 - 8 * E.n >= b_none                # lcp and da are gone too; text and anchors stay
    assert code_of(api, e.dup_prefix) == ESTATE and code_of(api, e.record_counts, [[0, 1]]) == ESTATE
    assert code_of(api, e.records_build) == ESTATE and raw(x, ok, all_, None, None, 0) == (ESTATE, 12345)
    x.close()
