"""Maximal and supermaximal repeats on the GPU (debwt_fm_repeats; EsaResult.repeats) against Definition 11 as repeat_ref.py
writes it out.  Everything is compared exactly: every geometry case with the three kinds at fanout 64 and at fanout 2 (deep
trees on tiny arrays), the staircase of a homopolymer with the bound that pins the logarithmic searches, the seeded read set
with its filters, capped builds, a build that kept the LCP array alone, and the protocol."""
import ctypes

import numpy as np
import pytest

import esa_ref as ER
import fm_definition as F
import repeat_ref as RR
from test_fm_esa_gpu import index_of

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, ERANGE = -1, -4, -5
CASES = F.geometry_cases()


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


def check_kinds(x, e, E, fanout, max_lcp=0, min_len=1):
    """the three kinds against the reference, and the statistics of each call"""
    every = RR.repeats(E, min_len=min_len, kind="intervals", max_lcp=max_lcp)
    stored = E.lcp(max_lcp)
    for kind in RR.KINDS:
        want = RR.repeats(E, min_len=min_len, kind=kind, max_lcp=max_lcp)
        got = e.repeats(min_len=min_len, kind=kind)
        assert got.dtype == RR.DTYPE and np.array_equal(got, want), kind
        st = x.repeat_stats()
        assert st["rows"] == E.n and st["fanout"] == fanout and st["levels"] == levels_of(E.n, fanout)
        assert st["tree_bytes"] == 8 * sum(_level_sizes(E.n, fanout)) and st["scratch_bytes"] > st["tree_bytes"]
        assert st["searched"] == int(np.count_nonzero((stored >= min_len) | ((stored == max_lcp) & (stored > 0))))
        assert st["intervals"] == len(every) and st["capped_intervals"] == RR.capped_intervals(E, max_lcp)
        assert st["representatives"] == st["intervals"] + st["capped_intervals"]
        assert st["maximal"] == int(np.count_nonzero(every["flags"] & RR.IS_MAXIMAL))
        assert st["supermaximal"] == int(np.count_nonzero(every["flags"] & RR.IS_SUPERMAXIMAL))
        assert st["reported"] == len(want) and st["search_steps"] <= st["wave_steps"]
        assert st["search_steps"] <= E.n * 3 * 2 * fanout * max(st["levels"], 1)
        if len(want):
            top = int(want["len"].max())
            assert st["longest_len"] == top and st["longest_row_lo"] == int(want["row_lo"][want["len"] == top].min())
        else:
            assert st["longest_len"] == 0 and st["longest_row_lo"] == 0
    return every


def _level_sizes(n, fanout):
    out = []
    while n > 1:
        n = -(-n // fanout)
        out.append(n)
    return out


# ---- every geometry case ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fanout", [64, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_geometry_cases(api, monkeypatch, name, fanout):
    E = ER.of_case(name)
    monkeypatch.setenv("DEBWT_FM_REPEAT_FANOUT", str(fanout))
    x = index_of(api, CASES[name], 32)
    e = x.esa()
    check_kinds(x, e, E, fanout)
    if name == "n33":
        assert x.repeat_stats()["levels"] == (6 if fanout == 2 else 1)
    x.close()


# ---- the bound that pins the logarithmic searches -----------------------------------------------------------------------

def test_search_bound_on_a_staircase(api):
    """One record of 20,000 'T': lcp falls by one from row to row, so every right search runs to the end of the array.  A
    search costs at most 2 F reads per level; a linear scan reads n^2 / 2 = 2 * 10^8 entries."""
    E = ER.of_homopolymer(20000)
    x = index_of(api, E.records, 32)
    e = x.esa()
    every = check_kinds(x, e, E, 64)
    assert len(every) == 19999 and int(np.count_nonzero(every["flags"] & RR.IS_SUPERMAXIMAL)) == 1
    e.repeats(min_len=1, kind="intervals")
    st = x.repeat_stats()
    bound = st["rows"] * 3 * 2 * 64 * st["levels"]
    print(f"search_steps {st['search_steps']}, bound {bound}, wave_steps {st['wave_steps']}")
    assert st["levels"] == 3 and st["fanout"] == 64 and 0 < st["search_steps"] <= bound < 100_000_000
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
    monkeypatch.setenv("DEBWT_FM_REPEAT_FANOUT", str(fanout))
    e = fm.esa(sa=True)
    check_kinds(fm, e, E, fanout)
    for min_len in (1, 20, 50):
        for min_occ, max_occ in ((2, None), (5, None), (2, 2), (2, 10), (5, 10)):
            for kind in ("maximal", "intervals"):
                want = RR.repeats(E, min_len=min_len, min_occ=min_occ, max_occ=max_occ, kind=kind)
                got = e.repeats(min_len=min_len, min_occ=min_occ, max_occ=max_occ, kind=kind)
                assert np.array_equal(got, want), (min_len, min_occ, max_occ, kind)
    mx, sp = e.repeats(min_len=1), e.repeats(min_len=1, kind="supermaximal")
    assert len(sp) and np.array_equal(sp, mx[(mx["flags"] & RR.IS_SUPERMAXIMAL) != 0])
    e.repeats(min_len=1)
    assert int(mx["len"].max()) == e.summary()["max"] == fm.repeat_stats()["longest_len"]
    # the occurrences of the longest repeat, from the kept suffix array, spell one string
    top = mx[int(np.argmax(mx["len"]))]
    pos = e.sa(int(top["row_lo"]), int(top["row_lo"] + top["count"]))
    words = {E.sym[int(p):int(p) + int(top["len"])].tobytes() for p in pos}
    assert len(words) == 1 and len(pos) == top["count"] and (E.sym[int(pos[0]):int(pos[0]) + int(top["len"])] <= 3).all()
    e.release()


# ---- caps ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_lcp", [1, 7, 40])
@pytest.mark.parametrize("name", ["dup_40x20", "homopolymer_only_one_record"])
def test_caps(api, name, max_lcp):
    E = ER.of_case(name)
    x = index_of(api, CASES[name], 32)
    e = x.esa(max_lcp=max_lcp)
    check_kinds(x, e, E, 64, max_lcp)
    st = x.repeat_stats()
    assert st["capped_intervals"] == RR.capped_intervals(E, max_lcp) and (st["capped_intervals"] > 0) == (max_lcp <= E.summary()["max"])
    assert len(e.repeats(min_len=max_lcp, kind="intervals")) == 0       # nothing of the capped value is reported
    assert x.repeat_stats()["capped_intervals"] == st["capped_intervals"]
    x.close()


@pytest.mark.parametrize("max_lcp", [1, 7, 40])
def test_caps_on_the_read_set(api, fm, max_lcp):
    E = ER.of_read_set()
    e = fm.esa(max_lcp=max_lcp)
    check_kinds(fm, e, E, 64, max_lcp)
    assert fm.repeat_stats()["capped_intervals"] == RR.capped_intervals(E, max_lcp) > 0
    e.release()


# ---- the LCP array alone ------------------------------------------------------------------------------------------------

def test_lcp_alone(api, fm):
    E = ER.of_read_set()
    e = fm.esa(sa=True, da=True)
    with_all = e.repeats(min_len=20)
    e = fm.esa()                                                        # neither sa nor da
    assert code_of(api, e.sa) == ESTATE and code_of(api, e.da) == ESTATE
    b0, lcp0 = fm.info()["device_bytes"], e.lcp()
    got = e.repeats(min_len=20)
    assert np.array_equal(got, with_all) and np.array_equal(got, RR.repeats(E, min_len=20)) and len(got) > 100
    assert np.array_equal(e.lcp(), lcp0) and np.array_equal(lcp0, E.lcp())
    assert fm.info()["device_bytes"] == b0
    e.release()


# ---- protocol -----------------------------------------------------------------------------------------------------------

def code_of(api, fn, *args, **kw):
    with pytest.raises(api.DebwtError) as err:
        fn(*args, **kw)
    return err.value.code


def raw(x, opts, out, capacity, count=True):
    from debwt_amd import _lib
    n = ctypes.c_uint64(12345)
    o = None if opts is None else ctypes.byref(_lib.DebwtFmRepeatOpts(*opts))
    p = None if out is None else out.ctypes.data_as(ctypes.c_void_p)
    rc = x._L.debwt_fm_repeats(x._h, o, p, capacity, ctypes.byref(n) if count else None)
    return rc, n.value


def test_protocol(api, monkeypatch):
    name = "n768"
    E = ER.of_case(name)
    x = index_of(api, CASES[name], 4)
    before = api.EsaResult(x)
    assert code_of(api, before.repeats, min_len=1) == ESTATE            # no build
    assert raw(x, (1, 0, 2, 0), None, 0) == (ESTATE, 12345)
    e = x.esa()
    want = RR.repeats(E, min_len=1)
    count = len(want)
    assert count > 10
    buf = np.zeros(count + 1, dtype=RR.DTYPE)
    ok = (1, 0, 2, 0)
    assert raw(x, None, None, 0)[0] == EINVAL and raw(x, ok, None, 0, count=False)[0] == EINVAL
    for bad in ((0, 0, 2, 0), (1, 0, 1, 0), (1, 0, 0, 0), (1, 0, 5, 4), (1, 3, 2, 0), (1, 0xFFFFFFFF, 2, 0)):
        assert raw(x, bad, None, 0) == (EINVAL, 12345), bad
    assert raw(x, ok, None, 1)[0] == EINVAL                             # no out with capacity > 0
    assert raw(x, (1, 0, 5, 5), None, 0)[0] in (0, ERANGE)              # max_occ == min_occ is a filter, not an error
    assert raw(x, ok, None, 0) == (ERANGE, count)                       # the sizing call
    assert raw(x, ok, buf, count - 1) == (ERANGE, count) and not buf.view(np.uint8).any()
    assert raw(x, ok, buf, count) == (0, count)
    assert np.array_equal(buf[:count], want) and not buf[count:].view(np.uint8).any()
    assert raw(x, (1, 0, 2, 0), buf, count + 1) == (0, count)
    assert raw(x, (10 ** 6, 0, 2, 0), None, 0) == (0, 0)                # nothing that long: the sizing call itself succeeds
    for fanout in ("3", "128", "1"):
        monkeypatch.setenv("DEBWT_FM_REPEAT_FANOUT", fanout)
        assert raw(x, ok, None, 0) == (EINVAL, 12345), fanout
    monkeypatch.delenv("DEBWT_FM_REPEAT_FANOUT")
    assert code_of(api, e.repeats, kind="intervals", min_occ=1) == EINVAL
    with pytest.raises(ValueError):
        e.repeats(kind="tandem")

    e = x.esa(max_lcp=5)                                                # a second build: the call reads the new array
    got = e.repeats(min_len=1, kind="intervals")
    assert np.array_equal(got, RR.repeats(E, min_len=1, kind="intervals", max_lcp=5)) and int(got["len"].max()) < 5
    assert x.repeat_stats()["capped_intervals"] == RR.capped_intervals(E, 5)
    e.release()
    assert code_of(api, e.repeats, min_len=1) == ESTATE and raw(x, ok, None, 0) == (ESTATE, 12345)
    x.close()
