"""Suffix array, LCP array and record array on the GPU (debwt_fm_esa_*; FMIndex.esa) against Definition 10 as esa_ref.py
writes it out.  Everything is compared exactly: every geometry case at sa_sample 1, 4, 32 and 1024, the seeded read set
with the spectrum as a second witness of the profile, caps, chunk lengths, the compare bound that pins the carry, an
index from files alone with its device bytes, and the protocol.

index_of(api, records, s) builds the index with the library's own builder where it takes the collection (every record
longer than 32 bases, as in fm_definition.BUILDER_CASES and the long outside-domain cases) and opens it from the
definition's rows and samples otherwise; neither way attaches a text, so every build here restores it first."""
import math

import numpy as np
import pytest

import esa_ref as ER
import fm_definition as F
from test_fm_search_gpu import index_of as built_index

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -4
CASES = F.geometry_cases()
SAMPLINGS = (1, 4, 32, 1024)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


@pytest.fixture(autouse=True)
def default_limits(monkeypatch):
    monkeypatch.delenv("DEBWT_FM_ESA_CHUNK", raising=False)


def opened(api, records, s, sa=None):
    if sa is None:
        sym, sa, L, words, hash_rows, dollar = F.definition_index(records)
    else:
        sym = F.text_symbols(records)
        L = sym[(sa - 1) % len(sym)]
        words, hash_rows, dollar = F.pack_rows(L), np.nonzero(L == F.SEP)[0].astype(np.uint64), int(np.nonzero(L == F.END)[0][0])
    return api.FMIndex.open(words, len(sym), hash_rows, dollar, F.samples(sa, s), sa_sample=s)


def index_of(api, records, s):
    if min(len(r) for r in records) > 32:
        return built_index(api, records, s)
    return opened(api, records, s)


def check_all(x, E, max_lcp=0):
    """one build with both flags: the three arrays, the summary and the profile"""
    e = x.esa(max_lcp=max_lcp, sa=True, da=True)
    sa, da, lcp = e.sa(), e.da(), e.lcp()
    assert sa.dtype == np.uint64 and da.dtype == np.uint32 and lcp.dtype == np.uint32
    assert np.array_equal(sa, E.sa.astype(np.uint64))
    assert np.array_equal(da, E.da)
    assert np.array_equal(lcp, E.lcp(max_lcp))
    assert e.summary() == E.summary(max_lcp)
    kmax = min(16, ER.cap_of(max_lcp))
    assert e.profile(kmax).tolist() == E.profile(kmax, max_lcp)
    return e


# ---- every geometry case ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", SAMPLINGS)
@pytest.mark.parametrize("name", list(CASES))
def test_geometry_cases(api, name, s):
    E = ER.of_case(name)
    x = index_of(api, CASES[name], s)
    check_all(x, E)
    st = x.esa_stats()
    assert st["walk_steps"] == E.n - 1 and st["walk_items"] >= 1 and st["walk_steps"] <= st["walk_wave_steps"]
    assert st["chunk_len"] == 256 and st["chunks"] == math.ceil(E.n / 256)
    assert st["symbols_compared"] % 32 == 0 and st["symbols_compared"] <= ER.compare_bound(E, 256)
    assert st["symbols_compared"] // 32 <= st["plcp_wave_steps"] or st["symbols_compared"] == 0
    assert st["kept_bytes"] == 16 * E.n and st["build_bytes"] >= 28 * E.n and st["ms_text"] > 0 and st["ms_wall"] > 0
    x.close()


# ---- the seeded read set ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fm(api):
    x = index_of(api, ER.of_read_set().records, 4)
    yield x
    x.close()


def test_read_set(api, fm):
    E = ER.of_read_set()
    e = check_all(fm, E)
    prof = e.profile(32)
    assert prof.tolist() == E.profile(32)
    for k in (1, 12, 13, 21, 32):
        assert int(prof[k - 1]) == fm.spectrum(k, strands="forward").distinct
    sm = e.summary()
    a, b = E.resolve(sm["pos_prev"]), E.resolve(sm["pos"])
    ra, rb = F.strings(E.records)[a[0]], F.strings(E.records)[b[0]]
    assert ra[a[1]:a[1] + sm["max"]] == rb[b[1]:b[1] + sm["max"]] and sm["max"] >= 50    # the longest repeat, in letters
    e.release()


# ---- caps ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_lcp", [1, 7, 40, 65535])
@pytest.mark.parametrize("name", ["dup_40x20", "homopolymer_only_one_record"])
def test_caps(api, name, max_lcp):
    E = ER.of_case(name)
    x = index_of(api, CASES[name], 32)
    e = check_all(x, E, max_lcp)
    sm, full = e.summary(), E.lcp_full
    assert sm["cap"] == max_lcp and sm["capped"] == int(np.count_nonzero(np.minimum(full, max_lcp) == max_lcp))
    assert (sm["capped"] > 0) == (max_lcp <= int(full.max())) and sm["max"] == min(int(full.max()), max_lcp)
    x.close()


# ---- chunk lengths ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["homopolymer_only_one_record", "dup_40x20", "n768"])
def test_chunk_lengths(api, monkeypatch, name):
    E = ER.of_case(name)
    x = index_of(api, CASES[name], 8)
    want = None
    for chunk in (None, 1, 64, E.n + 5):
        if chunk is not None:
            monkeypatch.setenv("DEBWT_FM_ESA_CHUNK", str(chunk))
        e = check_all(x, E)
        got = (e.sa().tobytes(), e.da().tobytes(), e.lcp().tobytes(), e.profile(16).tobytes())
        want = want or got
        assert got == want
        st = x.esa_stats()
        length = chunk or 256
        assert st["chunk_len"] == length and st["chunks"] == math.ceil(E.n / length)
        assert st["symbols_compared"] <= ER.compare_bound(E, length)
    x.close()


# ---- the bound that pins the carry --------------------------------------------------------------------------------------

def test_compare_bound_pins_the_carry(api, monkeypatch):
    """One record of 20,000 'T', chunks of 256 positions, no cap: plcp falls by one from position to position, so a walk
    that carries the match length compares about two words per position plus one restart per chunk; a walk that starts
    from 0 everywhere compares n^2 / 2 = 2 * 10^8 symbols."""
    E = ER.of_homopolymer(20000)
    monkeypatch.setenv("DEBWT_FM_ESA_CHUNK", "256")
    x = index_of(api, E.records, 32)
    check_all(x, E)
    st = x.esa_stats()
    bound = ER.compare_bound(E, 256)
    print(f"symbols_compared {st['symbols_compared']}, bound {bound}, sum of lcp {int(E.lcp_full.sum())}")
    assert 1_000_000 < bound < 3_000_000 and int(E.lcp_full.sum()) > 190_000_000
    assert st["chunks"] == math.ceil(E.n / 256) and 0 < st["symbols_compared"] <= bound
    x.close()


# ---- an index from files alone ------------------------------------------------------------------------------------------

def test_index_from_files(api):
    E = ER.of_read_set()
    n = E.n
    x, y = opened(api, E.records, 16, E.sa), opened(api, E.records, 16, E.sa)
    b0 = x.info()["device_bytes"]
    assert y.info()["device_bytes"] == b0
    y.restore_text()
    text_bytes = y.info()["device_bytes"] - b0                          # the text and the anchors of the restore
    assert text_bytes >= ((n + 63) // 32 + 2) * 8
    y.close()
    e = check_all(x, E)
    b1 = x.info()["device_bytes"]
    assert b1 - b0 == text_bytes + 16 * n and x.esa_stats()["kept_bytes"] == 16 * n
    e = x.esa()                                                         # lcp alone; the text is attached now
    assert x.info()["device_bytes"] - b0 == text_bytes + 4 * n and x.esa_stats()["ms_text"] == 0
    assert np.array_equal(e.lcp(), E.lcp())
    e.release()
    assert x.info()["device_bytes"] - b0 == text_bytes
    x.close()


# ---- protocol -----------------------------------------------------------------------------------------------------------

def code_of(api, fn, *args, **kw):
    with pytest.raises(api.DebwtError) as err:
        fn(*args, **kw)
    return err.value.code


def test_protocol(api):
    E = ER.of_case("n768")
    n = E.n
    x = index_of(api, CASES["n768"], 4)
    before = api.EsaResult(x)
    for fn in (before.lcp, before.sa, before.da, before.summary):
        assert code_of(api, fn) == ESTATE
    assert code_of(api, before.profile, 4) == ESTATE
    x._chk(x._L.debwt_fm_esa_release(x._h))                              # nothing to release: OK
    b0 = x.info()["device_bytes"]
    assert code_of(api, lambda: x._chk(x._L.debwt_fm_esa_build(x._h, 0, 4))) == EINVAL     # unknown flag
    assert code_of(api, before.lcp) == ESTATE

    e = x.esa(sa=True)
    sa, lcp = E.sa.astype(np.uint64), E.lcp()
    assert e.sa(0, 1).tolist() == [sa[0]] and e.sa(n - 1, n).tolist() == [sa[n - 1]]
    assert np.array_equal(e.lcp(380, 390), lcp[380:390]) and np.array_equal(e.sa(383, 386), sa[383:386])
    assert len(e.lcp(5, 5)) == 0 and len(e.sa(n, n)) == 0 and len(e.lcp(0, 0)) == 0
    assert x._L.debwt_fm_esa_fetch(x._h, 0, 7, 0, None) == 0            # count 0 needs no destination
    assert code_of(api, e.da) == ESTATE                                 # not kept
    assert code_of(api, e.lcp, n - 1, n + 1) == EINVAL and code_of(api, e.sa, n + 1, n + 1) == EINVAL
    assert code_of(api, lambda: x._chk(x._L.debwt_fm_esa_fetch(x._h, 3, 0, 1, None))) == EINVAL
    assert code_of(api, e.profile, 4097) == EINVAL and code_of(api, e.profile, 0) == EINVAL
    assert len(e.profile(4096)) == 4096 and e.profile(4096)[-1] == 0

    e = x.esa(max_lcp=5, da=True)                                       # a rebuild with other flags replaces the first
    assert code_of(api, e.sa) == ESTATE and np.array_equal(e.da(), E.da) and np.array_equal(e.lcp(), E.lcp(5))
    assert code_of(api, e.profile, 6) == EINVAL and e.profile(5).tolist() == E.profile(5, 5)
    assert x.info()["device_bytes"] - b0 >= 8 * n                       # lcp and da, and the text of the first build
    e.release()
    for fn in (e.lcp, e.da, e.summary):
        assert code_of(api, fn) == ESTATE
    e.release()                                                         # twice: OK
    x.close()


def test_samples_of_other_rows_are_refused(api):
    """two samples swapped before FMIndex.open: DEBWT_EINVAL, nothing kept -- a refused input, not a fault"""
    name = "n1152_single"                                               # one record: opening locates nothing
    D, E = F.definition_of(name), ER.of_case(name)
    samples = F.samples(D.sa, 4)
    samples[[3, 7]] = samples[[7, 3]]
    x = api.FMIndex.open(D.words, D.n, D.hash_rows, D.dollar_row, samples, sa_sample=4)
    b0 = x.info()["device_bytes"]
    assert code_of(api, x.esa, sa=True, da=True) == EINVAL
    assert code_of(api, api.EsaResult(x).lcp) == ESTATE and code_of(api, api.EsaResult(x).summary) == ESTATE
    assert x.esa_stats()["kept_bytes"] == 0
    assert x.info()["device_bytes"] - b0 < 4 * D.n                      # the anchors at most: no array, no text
    x.close()
    x = api.FMIndex.open(D.words, D.n, D.hash_rows, D.dollar_row, F.samples(D.sa, 4), sa_sample=4)
    check_all(x, E)                                                     # the same files with their own samples
    x.close()
