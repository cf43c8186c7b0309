"""k-mer counts along reads (debwt_fm_kmer_counts, FMIndex.kmer_counts) against the reference of kmer_ref.py, compared
exactly: the seeded read set against its own index with the edge patterns, every k that takes another path through the
prefix table, both strands, the existing count path, table sizes, batches, goldens, an index from files, errors and
statistics."""
import ctypes

import numpy as np
import pytest

import kmer_ref as KR
from conftest import golden_outputs, golden_records
from overlap_ref import codes
from test_fm_index_gpu import text_of
from test_fm_search_gpu import entry_named, index_of

pytestmark = pytest.mark.gpu


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
    monkeypatch.delenv("DEBWT_FM_KMER_ITEMS", raising=False)


def check(res, pats, R):
    assert len(res) == len(pats)
    k = R.k
    want_off = np.concatenate([[0], np.cumsum([max(0, len(p) - k + 1) for p in pats])])
    assert np.array_equal(res.offsets, want_off.astype(np.uint64))
    for i, p in enumerate(pats):
        assert res.profile(i).tolist() == R.profile(p), (i, p)
    assert res.counts.dtype == np.uint32 and len(res.counts) == int(want_off[-1])


@pytest.mark.parametrize("strands", ["forward", "both"])
@pytest.mark.parametrize("k", [1, 4, 11, 16, 31])
def test_read_set(api, fm, k, strands):
    pats = KR.kmer_queries(k)
    R = KR.ref_of(k, strands == "both")
    res = fm.kmer_counts(pats, k, strands=strands)
    check(res, pats, R)
    if strands == "both" and k in (4, 16):                      # its own reverse complement: counted twice
        w = "ACGT" if k == 4 else KR.read_set()["palindrome"]
        assert KR.revcomp(w) == w and R.cnt(w) == 2 * R.occ(w) > 0
    st = fm.kmer_stats()
    assert st["patterns"] == len(pats) and st["batches"] == 1 and st["kmers"] == len(res.counts)
    assert 0 < st["steps"] <= st["wave_steps"] and st["line_reads"] >= st["steps"]
    assert st["ms_kernel"] > 0 and st["ms_wall"] > 0 and st["scratch_bytes"] > 0 and st["launches"] >= 1


def test_profile_is_count_of_the_exploded_list(api, fm):
    k = 11
    pats = KR.kmer_queries(k)
    res = fm.kmer_counts(pats, k)
    flat = [p[j:j + k] for p in pats for j in range(len(p) - k + 1)]
    assert len(flat) == len(res.counts)
    cnt = fm.count(flat)
    assert np.array_equal(res.counts.astype(np.uint64), cnt) and int(cnt.sum()) > 0


def test_table_sizes(api, monkeypatch):
    """q in {0, 3, 4, 6} against k in {1, 4, 11}: k < q, k = q and k > q.  The table is made by the first call that needs
    it (q > 0 and k >= q), replaced when such a call finds another q, and counted in device_bytes from then on."""
    own = index_of(api, codes(KR.read_set()["records"]), s=4)
    base = own.info()["device_bytes"]
    want, kept = {}, 0
    for q in (0, 3, 4, 6):
        monkeypatch.setenv("DEBWT_FM_KMER_TABLE_Q", str(q))
        for k in (1, 4, 11):
            pats = KR.kmer_queries(k)
            for strands in ("forward", "both"):
                assert own.info()["device_bytes"] == base + (16 * 4 ** kept if kept else 0)      # only after the call
                res = own.kmer_counts(pats, k, strands=strands)
                st = own.kmer_stats()
                if q == 0:
                    want[k, strands] = res
                    check(res, pats, KR.ref_of(k, strands == "both"))
                assert np.array_equal(res.counts, want[k, strands].counts), (q, k, strands)
                used = q if k >= q else 0
                built = used and used != kept
                kept = used or kept
                assert st["table_q"] == used and (st["ms_table"] > 0) == bool(built)
                assert own.info()["device_bytes"] == base + (16 * 4 ** kept if kept else 0)
                # one start per k-mer and strand whose last q characters are bases
                if not used:
                    assert st["table_starts"] == 0
                else:
                    ok = lambda w: all(c in "ACGTacgt" for c in w)                             # noqa: E731
                    good = sum(ok(p[j + k - q:j + k]) + (strands == "both" and ok(p[j:j + q]))
                               for p in pats for j in range(len(p) - k + 1))
                    assert st["table_starts"] == good > 0
    assert kept == 6
    monkeypatch.setenv("DEBWT_FM_KMER_TABLE_Q", "13")
    with pytest.raises(api.DebwtError) as e:
        own.kmer_counts(["ACGT"], 2)
    assert e.value.code == -1
    own.close()


def test_batches_do_not_change_results(api, fm, monkeypatch):
    k = 16
    pats = KR.kmer_queries(k)
    ref = fm.kmer_counts(pats, k, strands="both")
    assert fm.kmer_stats()["batches"] == 1
    for items in ("7", "1000"):
        monkeypatch.setenv("DEBWT_FM_KMER_ITEMS", items)
        got = fm.kmer_counts(pats, k, strands="both")
        st = fm.kmer_stats()
        assert np.array_equal(got.offsets, ref.offsets) and np.array_equal(got.counts, ref.counts)
        assert st["batches"] > 1 and st["kmers"] == len(ref.counts)


def rec_strings(recs):
    return ["".join("ACGT"[c] for c in np.asarray(r).tolist()) for r in recs]


@pytest.mark.parametrize("k", [12, 32])
@pytest.mark.parametrize("name", ["shared_ends_duplicates", "special_branches"])
def test_goldens(api, name, k):
    recs = golden_records(entry_named(name))
    strs = rec_strings(recs)
    rng = np.random.default_rng(3)
    pats = [s[:300] for s in strs][:200] + [KR.revcomp(s[:90]) for s in strs[:50]] + [KR.rand_dna(rng, 60), "", strs[0][:k - 1]]
    fm = index_of(api, recs)
    for strands in ("forward", "both"):
        check(fm.kmer_counts(pats, k, strands=strands), pats, KR.Ref(strs, k, strands == "both"))
    fm.close()


def test_index_from_files(api):
    entry = entry_named("shared_ends_duplicates")
    recs = golden_records(entry)
    strs = rec_strings(recs)
    text, _ = text_of(recs)
    words, hrows, drow = golden_outputs(entry)
    own = index_of(api, recs, s=4)
    opened = api.FMIndex.open(words, len(text), hrows, drow, own.samples(), sa_sample=4)     # no text is ever attached
    pats = [s[:200] for s in strs] + ["", "acgtn"]
    before = opened.info()["device_bytes"]
    a = own.kmer_counts(pats, 14, strands="both")
    b = opened.kmer_counts(pats, 14, strands="both")
    check(b, pats, KR.Ref(strs, 14, True))
    assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.counts, b.counts) and int(a.counts.sum()) > 0
    after = opened.info()["device_bytes"]
    assert after == before + 16 * 4 ** opened.kmer_stats()["table_q"] and opened.kmer_stats()["table_q"] > 0
    opened.kmer_counts(pats, 14)
    assert opened.info()["device_bytes"] == after
    own.close(); opened.close()


def test_errors_and_capacity(api, fm):
    from debwt_amd import _lib
    k = 11
    pats = [p.encode() for p in KR.kmer_queries(k)[-40:]]
    buf = b"".join(pats)
    n = len(pats)
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in pats], out=offs[1:])
    L = _lib.lib()
    coff = np.zeros(n + 1, dtype=np.uint64)
    u32p = ctypes.POINTER(ctypes.c_uint32)

    def call(o, k, flags, cap, null=False):
        c = np.zeros(max(cap, 1), dtype=np.uint32)
        rc = L.debwt_fm_kmer_counts(fm._h, buf, api._p64(o), n, k, flags, api._p64(coff), None if null else c.ctypes.data_as(u32p), cap)
        return rc, c

    res = fm.kmer_counts(pats, k, strands="both")
    total = len(res.counts)
    assert total > n
    assert call(offs, 0, 0, total)[0] == -1
    assert call(offs, k, 2, total)[0] == -1 and call(offs, k, 4 | 1, total)[0] == -1
    bad = offs.copy()
    bad[3] = bad[4] + 1
    assert call(bad, k, 0, total)[0] == -1
    with pytest.raises(api.DebwtError) as e:
        fm.kmer_counts(["ACGT"], 0)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        fm.kmer_counts(["ACGT"], 2, strands="reverse")
    for cap, null in ((0, True), (total - 1, False)):
        coff[:] = 0
        assert call(offs, k, 1, cap, null)[0] == -5 and np.array_equal(coff, res.offsets)      # written first
    rc, c = call(offs, k, 1, total)
    assert rc == 0 and np.array_equal(coff, res.offsets) and np.array_equal(c, res.counts)
    empty = fm.kmer_counts([], 5)
    assert len(empty) == 0 and len(empty.counts) == 0
    assert len(fm.kmer_counts(["ACGT", ""], 5).counts) == 0
