"""The k-mer spectrum of the indexed collection (debwt_fm_spectrum, debwt_fm_kmer_list; FMIndex.spectrum, kmer_list,
correct(min_count="auto")) against Definition 9 as spectrum_ref.py writes it out, compared exactly: the seeded read set
at every k that takes another path (k < q, k = q, k = q + 1, the top bits of the code at k = 32, k-mers equal to their
reverse complement at k = 4 and 16), the definition-built edge collections, chunk limits and table sizes, bins, list
filters, the capacity protocol, errors, statistics and an index from files."""
import ctypes
import inspect

import numpy as np
import pytest

import fm_definition as F
import kmer_ref as KR
import spectrum_ref as SR
from overlap_ref import codes
from test_fm_search_gpu import index_of

pytestmark = pytest.mark.gpu
EINVAL, ERANGE = -1, -5
CASES = F.geometry_cases()
BOTH = 1
DEFAULT_ITEMS = 1 << 22


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


@pytest.fixture(scope="module")
def fm(api):
    """the index of the seeded read set: built once, queried by every test below and never changed"""
    x = index_of(api, codes(KR.read_set()["records"]), s=4)
    yield x
    x.close()


@pytest.fixture(autouse=True)
def default_limits(monkeypatch):
    monkeypatch.delenv("DEBWT_FM_KMER_TABLE_Q", raising=False)
    monkeypatch.delenv("DEBWT_FM_SPECTRUM_ITEMS", raising=False)


def check_spectrum(sp, D, nbins):
    distinct, total, over = SR.totals(D, nbins)
    assert sp.hist.dtype == np.uint64 and sp.hist.tolist() == SR.histogram(D, nbins)
    assert (sp.distinct, sp.total, sp.overflow_total) == (distinct, total, over)


def check_list(got, D, min_mult=1, max_mult=SR.U32_MAX):
    cs, ms = got
    want = SR.listing(D, min_mult, max_mult)
    assert cs.dtype == np.uint64 and ms.dtype == np.uint32
    assert cs.tolist() == [c for c, _ in want] and ms.tolist() == [m for _, m in want]
    assert len(cs) < 2 or bool((cs[1:] > cs[:-1]).all())           # strictly ascending


def check_both_ways(x, strs, k, bins=256):
    """spectrum and full list of one index on both strand settings"""
    for strands in ("forward", "both"):
        D = SR.members(strs, k, strands == "both")
        check_spectrum(x.spectrum(k, strands=strands, bins=bins), D, bins)
        check_list(x.kmer_list(k, strands=strands), D)


# ---- the seeded read set ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strands", ["forward", "both"])
@pytest.mark.parametrize("k", [1, 4, 11, 12, 13, 16, 21, 31, 32])
def test_read_set(api, fm, k, strands):
    both = strands == "both"
    D = SR.of_read_set(k, both)
    sp = fm.spectrum(k, strands=strands)
    st = fm.spectrum_stats()
    check_spectrum(sp, D, 256)
    assert st["leaves"] >= sp.distinct > 0 and st["chunks"] >= 1 and st["ms_kernel"] > 0 and st["ms_wall"] > 0
    assert st["table_q"] == (12 if k >= 12 else 0) and st["levels"] == k - st["table_q"]
    assert st["level_intervals"][k] == st["leaves"] == len(SR.of_read_set(k, False))     # every forward k-mer is a leaf
    assert sum(st["level_intervals"][:k]) == st["expanded"]
    assert st["steps"] <= st["wave_steps"] and st["line_reads"] >= st["steps"]
    assert (st["steps"] > 0) == (st["levels"] > 0)                  # k = q: the table's entries are the leaves
    if both:
        pal = sum(1 for c in SR.of_read_set(k, False) if KR.revcomp(SR.string_of(c, k)) == SR.string_of(c, k))
        assert st["lookups"] == st["leaves"] - pal and (pal > 0 or k not in (4, 16)) and (pal == 0 or k % 2 == 0)
    else:
        assert st["lookups"] == 0 and st["steps"] == st["expanded"]
    cs, ms = got = fm.kmer_list(k, strands=strands)
    check_list(got, D)
    words = [api.kmer_string(c, k) for c in cs.tolist()]
    assert words == [SR.string_of(c, k) for c in cs.tolist()]
    if both:
        assert np.array_equal(fm.kmer_counts(words, k, strands="both").counts, ms)
        if k == 16:                                                   # the planted 16-mer: counted twice
            pal = KR.read_set()["palindrome"]
            assert D[SR.code_of(pal)] == 2 * int(fm.count([pal])[0]) > 0
    else:
        assert np.array_equal(fm.count(words), ms.astype(np.uint64))
    if k == 32:
        assert int(cs.max()) >> 62 == 3 and int(cs.min()) >> 62 == 0      # the top digit of the code is in use


def test_threshold_of_the_read_set(api, fm):
    for k, strands, valley, peak in ((15, "both", 6, 22), (21, "both", 5, 19), (31, "both", 3, 13), (15, "forward", 3, 9)):
        sp = fm.spectrum(k, strands=strands)
        t = sp.threshold()
        assert (t["valley"], t["peak"]) == (valley, peak) and t == api.spectrum_threshold(sp.hist, sp.total)
        assert t["est_size"] == SR.threshold(sp.hist.tolist(), sp.total)[2]
    assert fm.spectrum(1).threshold() == {"valley": 0, "peak": 0, "est_size": 0}


# ---- edge collections ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_edge_collections(api, name):
    D = F.definition_of(name)
    x = api.FMIndex.open(D.words, D.n, D.hash_rows, D.dollar_row, F.samples(D.sa, 32), sa_sample=32)
    for k in (1, 2, 3, 8, 32):
        check_both_ways(x, D.strs, k)
    if name == "ones_600":                                          # records of one base: no 2-mer exists
        sp = x.spectrum(2)
        assert sp.distinct == sp.total == 0 and not sp.hist.any() and len(x.kmer_list(2)[0]) == 0
        assert x.spectrum_stats()["leaves"] == 0
    if name == "all_T_x3":
        assert [a.tolist() for a in x.kmer_list(2)] == [[0], [435]]          # T^2 under the code of A^2
        assert [a.tolist() for a in x.kmer_list(2, strands="forward")] == [[15], [435]]
    x.close()


@pytest.mark.parametrize("name", F.BUILDER_CASES)
def test_builder_cases(api, name):
    D = F.definition_of(name)
    x = index_of(api, D.records, s=32)
    for k in (3, 8, 32):
        check_both_ways(x, D.strs, k)
    x.close()


# ---- limits -------------------------------------------------------------------------------------------------------------

def chunks_of(sizes, limit):
    """the number of chunks: the start entries in table order, cut so that a chunk's sizes sum to at most limit; an entry
    above the limit goes alone"""
    chunks, s = 0, 0
    for x in sizes:
        if s and s + x > limit:
            chunks, s = chunks + 1, 0
        s += x
        if s >= limit:
            chunks, s = chunks + 1, 0
    return chunks + (1 if s else 0)


@pytest.mark.parametrize("q", [0, 3, 6, 12])
def test_no_result_depends_on_the_limits(api, q, monkeypatch):
    strs = KR.read_set()["records"]
    own = index_of(api, codes(strs), s=4)
    base = own.info()["device_bytes"]
    n = own.info()["n"]
    monkeypatch.setenv("DEBWT_FM_KMER_TABLE_Q", str(q))
    for k in (4, 21):
        used = q if k >= q else 0
        starts = SR.members(strs, used, False) if used else {0: n}       # the start entries and their sizes
        largest, mass = max(starts.values()), sum(starts.values())
        for items in (1, 64, 1000, None):
            if items is None:
                monkeypatch.delenv("DEBWT_FM_SPECTRUM_ITEMS")
            else:
                monkeypatch.setenv("DEBWT_FM_SPECTRUM_ITEMS", str(items))
            limit = items or DEFAULT_ITEMS
            bound = 60 * max(limit, largest) + 16 * ((4 ** used + 1023) // 1024 if used else 0) + (1 << 20)
            full = items in (1000, None) or k == 4                  # thousands of chunks of nine levels: one call is enough
            for strands in ("forward", "both") if full else ("both",):
                D = SR.of_read_set(k, strands == "both")
                check_spectrum(own.spectrum(k, strands=strands), D, 256)
                st = own.spectrum_stats()
                assert st["table_q"] == used and st["items_limit"] == limit and 0 < st["scratch_bytes"] <= bound
                assert st["chunks"] == chunks_of([starts[c] for c in sorted(starts)], limit)
                if items == 1 and used:
                    assert st["chunks"] == len(starts) > 1              # every start entry goes alone
                assert (st["chunks"] > 1) == (used > 0 and mass > limit)
                assert own.info()["device_bytes"] == base + (16 * 4 ** used if used else 0)
            if full:
                check_list(own.kmer_list(k), SR.of_read_set(k, True))
                assert 0 < own.spectrum_stats()["scratch_bytes"] <= bound
    monkeypatch.setenv("DEBWT_FM_KMER_TABLE_Q", "13")
    with pytest.raises(api.DebwtError) as e:
        own.spectrum(4)
    assert e.value.code == EINVAL
    own.close()


# ---- bins, filters, capacity, errors ------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", [2, 3, 256, 4096])
def test_bins(api, fm, bins):
    for k, strands in ((1, "both"), (4, "forward"), (21, "both")):
        D = SR.of_read_set(k, strands == "both")
        sp = fm.spectrum(k, strands=strands, bins=bins)
        check_spectrum(sp, D, bins)
        assert len(sp.hist) == bins and int(sp.hist.sum()) == sp.distinct
        if bins == 2:
            assert sp.hist.tolist() == [0, sp.distinct] and sp.overflow_total == sp.total
        if bins == 4096 and k == 21:
            assert sp.overflow_total == 0
    if bins == 256:
        assert fm.spectrum(1, bins=256).overflow_total == fm.spectrum(1).total > 0       # single bases: all in the last bin


def test_list_filters(api, fm):
    k = 21
    D = SR.of_read_set(k, True)
    valley = fm.spectrum(k).threshold()["valley"]
    assert valley == 5
    for lo, hi in ((1, 1), (valley, 2 ** 32 - 1), (2, 4), (19, 19), (1, 2 ** 32 - 1)):
        got = fm.kmer_list(k, min_count=lo, max_count=hi)
        check_list(got, D, lo, hi)
        assert len(got[0]) > 0
    top = max(D.values())
    for lo, hi in ((top + 1, 2 ** 32 - 1), (top + 1, top + 1)):
        got = fm.kmer_list(k, min_count=lo, max_count=hi)
        assert len(got[0]) == 0 and len(got[1]) == 0
    solid = fm.kmer_list(k, min_count=valley)
    weak = fm.kmer_list(k, max_count=valley - 1)
    assert len(solid[0]) + len(weak[0]) == len(D)
    Df = SR.of_read_set(4, False)
    check_list(fm.kmer_list(4, strands="forward", min_count=300, max_count=500), Df, 300, 500)


def raw_list(api, fm, k, flags, lo, hi, cap, null=False, count=True):
    from debwt_amd import _lib
    L = _lib.lib()
    cs, ms, n = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint32), ctypes.c_uint64(2 ** 64 - 1)
    rc = L.debwt_fm_kmer_list(fm._h, k, flags, lo, hi, None if null else api._p64(cs),
                              None if null else ms.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap,
                              ctypes.byref(n) if count else None)
    return rc, n.value, cs, ms


def test_capacity_protocol(api, fm):
    k = 13
    want = SR.listing(SR.of_read_set(k, True), 2)
    total = len(want)
    assert total > 1000
    for cap, null in ((0, True), (1, False), (total - 1, False)):
        rc, n, _, _ = raw_list(api, fm, k, BOTH, 2, 2 ** 32 - 1, cap, null)
        assert rc == ERANGE and n == total, (cap, rc, n)             # count is written, the call comes back for more
    for cap in (total, total + 7):
        rc, n, cs, ms = raw_list(api, fm, k, BOTH, 2, 2 ** 32 - 1, cap)
        assert rc == 0 and n == total
        assert cs[:n].tolist() == [c for c, _ in want] and ms[:n].tolist() == [m for _, m in want]
    rc, n, _, _ = raw_list(api, fm, k, BOTH, 10 ** 6, 10 ** 6, 0, null=True)          # no member: capacity 0 is enough
    assert rc == 0 and n == 0


def test_errors(api, fm):
    from debwt_amd import _lib
    L = _lib.lib()
    hist = np.zeros(4097, dtype=np.uint64)
    tot = _lib.DebwtFmSpectrumTotals()

    def spec(k, flags, nbins, h=hist, t=tot, handle=fm._h):
        return L.debwt_fm_spectrum(handle, k, flags, nbins, api._p64(h) if h is not None else None,
                                   ctypes.byref(t) if t is not None else None)

    assert spec(21, BOTH, 256) == 0
    for k in (0, 33, 2 ** 31):
        assert spec(k, BOTH, 256) == EINVAL
        assert raw_list(api, fm, k, BOTH, 1, 5, 0, null=True)[0] == EINVAL
    for nbins in (0, 1, 4097):
        assert spec(21, BOTH, nbins) == EINVAL
    for flags in (2, 4 | 1, 2 ** 31):
        assert spec(21, flags, 256) == EINVAL
        assert raw_list(api, fm, 21, flags, 1, 5, 0, null=True)[0] == EINVAL
    assert spec(21, BOTH, 256, h=None) == EINVAL and spec(21, BOTH, 256, t=None) == EINVAL
    assert spec(21, BOTH, 256, handle=None) == EINVAL
    assert raw_list(api, fm, 21, BOTH, 0, 5, 0, null=True)[0] == EINVAL            # min_mult = 0
    assert raw_list(api, fm, 21, BOTH, 6, 5, 0, null=True)[0] == EINVAL            # min_mult > max_mult
    assert raw_list(api, fm, 21, BOTH, 1, 5, 10, null=True)[0] == EINVAL           # capacity without arrays
    assert raw_list(api, fm, 21, BOTH, 1, 5, 0, null=True, count=False)[0] == EINVAL
    assert L.debwt_fm_spectrum_stats_get(fm._h, None) == EINVAL and L.debwt_fm_spectrum_stats_get(None, None) == EINVAL
    with pytest.raises(api.DebwtError) as e:
        fm.spectrum(0)
    assert e.value.code == EINVAL and "k must be" in str(e.value)
    with pytest.raises(api.DebwtError):
        fm.spectrum(21, bins=1)
    with pytest.raises(api.DebwtError):
        fm.kmer_list(21, min_count=0)
    for call in (lambda: fm.spectrum(21, strands="reverse"), lambda: fm.kmer_list(21, strands="reverse")):
        with pytest.raises(ValueError):
            call()
    check_spectrum(fm.spectrum(21), SR.of_read_set(21, True), 256)                  # the index still answers


# ---- files --------------------------------------------------------------------------------------------------------------

def test_index_from_files(api, fm):
    strs = KR.read_set()["records"]
    d = api.DeBWT(k=32)
    d.load_records(codes(strs))
    d.build()
    words, hrows, drow = d.fetch()
    d.close()
    opened = api.FMIndex.open(words, fm.n, hrows, drow, fm.samples(), sa_sample=4)       # no text is ever attached
    before = opened.info()["device_bytes"]
    for k, strands in ((21, "both"), (31, "forward"), (4, "both")):
        D = SR.of_read_set(k, strands == "both")
        a, b = fm.spectrum(k, strands=strands), opened.spectrum(k, strands=strands)
        check_spectrum(b, D, 256)
        assert np.array_equal(a.hist, b.hist) and (a.distinct, a.total) == (b.distinct, b.total)
        check_list(opened.kmer_list(k, strands=strands, min_count=2), D, 2)
    assert opened.info()["device_bytes"] == before + 16 * 4 ** 12
    opened.close()


# ---- correct(min_count="auto") ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [15, 21])
def test_correct_auto(api, fm, k):
    D = SR.of_read_set(k, True)
    valley = SR.threshold(SR.histogram(D, 256), SR.totals(D, 256)[1])[0]
    assert valley == {15: 6, 21: 5}[k]
    pats = KR.correction_queries(k)
    out_a, info_a = fm.correct(pats, k, min_count="auto")
    out_v, info_v = fm.correct(pats, k, min_count=valley)
    assert out_a == out_v and np.array_equal(info_a, info_v)
    want = [KR.ref_of(k, True).correct(p, valley, 4) for p in pats[-10:]]
    assert [o.decode() for o in out_a[-10:]] == [w[0] for w in want]
    assert int(info_a["fixes"].sum()) > 0
    assert inspect.signature(api.FMIndex.correct).parameters["min_count"].default == 3      # the default stays 3
    Df = SR.of_read_set(k, False)
    vf = SR.threshold(SR.histogram(Df, 256), SR.totals(Df, 256)[1])[0]
    out_f, info_f = fm.correct(pats, k, min_count="auto", strands="forward")
    out_w, info_w = fm.correct(pats, k, min_count=vf, strands="forward")
    assert vf > 0 and out_f == out_w and np.array_equal(info_f, info_w)
    with pytest.raises(ValueError):
        fm.correct(pats, k, min_count="valley")


def test_correct_auto_without_a_valley(api):
    rng = np.random.default_rng(17)
    strs = [KR.rand_dna(rng, 60) for _ in range(40)]                # error free, coverage 1: every 15-mer occurs once
    x = index_of(api, codes(strs), s=4)
    sp = x.spectrum(15)
    assert sp.hist[1] == sp.distinct > 0 and sp.threshold()["valley"] == 0
    with pytest.raises(ValueError) as e:
        x.correct(strs, 15, min_count="auto")
    assert "spectrum" in str(e.value)
    out, info = x.correct(strs, 15, min_count=1)
    assert [o.decode() for o in out] == strs
    x.close()
