"""Suffix-prefix overlaps with mismatches (debwt_fm_overlaps_mm, FMIndex.overlaps_mm) against the reference of
overlap_mm_ref.py: the whole ordered hit list of every query, flags and mismatch counts included, compared exactly -- on
the mutated synthetic read set, on both strands, with the rate rule, the longest reduction, tiny buffers and batches,
errors and the capacity protocol, an index from files, statistics, and 20,000 golden reads."""
import ctypes

import numpy as np
import pytest

from conftest import golden_outputs, golden_records
from overlap_mm_ref import brute, mutated_reads, queries
from overlap_ref import CONTAINS, WHOLE, codes, extra_queries, longest_of, rand_dna, revcomp
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
def synth(api):
    """(mutated record strings, originals, the 165 queries, the index): built once, never changed"""
    strs, orig = mutated_reads()
    fm = index_of(api, codes(strs), s=4)
    yield strs, orig, queries(strs, orig, 20), fm
    fm.close()


_want = {}


def want_of(strs, pats, min_overlap, K, permille=0):
    """brute of every pattern, computed once per argument set and shared"""
    key = (id(pats), len(pats), min_overlap, K, permille)
    if key not in _want:
        _want[key] = (pats, [brute(strs, p, min_overlap, K, permille) for p in pats])
    return _want[key][1]


def tuples(res, i):
    return [tuple(int(x) for x in h) for h in res.hits(i).tolist()]


def check(res, pats, want):
    assert len(res) == len(pats)
    for i, p in enumerate(pats):
        got = tuples(res, i)
        assert got == want[i], (i, p)
        assert len({h[:3] for h in got}) == len(got)          # no (record, length, strand) twice
    assert int(res.count().sum()) == sum(len(w) for w in want) == len(res.all_hits)
    assert np.array_equal(res.mismatches(), (res.all_hits["flags"] >> 8).astype(np.uint8))


def same(a, b):
    return np.array_equal(a.offsets, b.offsets) and np.array_equal(a.all_hits, b.all_hits)


@pytest.mark.parametrize("min_overlap", [1, 20])
def test_zero_mismatches_is_overlaps(api, synth, min_overlap):
    strs, _, _, fm = synth
    pats = strs + extra_queries(strs, min_overlap)
    for strands in ("forward", "both"):
        for longest in (False, True):
            a = fm.overlaps(pats, min_overlap=min_overlap, strands=strands, longest=longest)
            b = fm.overlaps_mm(pats, min_overlap=min_overlap, mismatches=0, strands=strands, longest=longest)
            assert len(a.all_hits) > len(strs)
            assert same(a, b), (strands, longest)
            assert not a.mismatches().any() and not b.mismatches().any()


@pytest.mark.parametrize("K,min_overlap", [(1, 20), (2, 20), (3, 20), (1, 8)])
def test_against_the_definition(api, synth, K, min_overlap):
    strs, _, pats, fm = synth
    want = want_of(strs, pats, min_overlap, K)
    res = fm.overlaps_mm(pats, min_overlap=min_overlap, mismatches=K)
    check(res, pats, want)
    mm = res.mismatches()
    assert all(int((mm == k).sum()) > 0 for k in range(K + 1)) and int(mm.max()) == K


@pytest.mark.parametrize("permille", [25, 50])
def test_rate(api, synth, permille):
    strs, _, pats, fm = synth
    want = want_of(strs, pats, 20, 4, permille)
    res = fm.overlaps_mm(pats, min_overlap=20, mismatches=4, error_permille=permille)
    check(res, pats, want)
    free = len(fm.overlaps_mm(pats, min_overlap=20, mismatches=4).all_hits)
    assert len(res.all_hits) < free if permille == 25 else len(res.all_hits) <= free
    assert int(res.mismatches().max()) >= 1


def test_both_strands(api, synth):
    strs, orig, _, fm = synth
    rng = np.random.default_rng(7)
    pats = strs[::3] + [revcomp(s) for s in strs[1::5]] + [revcomp(s) for s in orig[2::31]] + extra_queries(strs, 20)
    pats += [revcomp(strs[6])[:50] + rand_dna(rng, 30), revcomp(strs[7][:33]).lower() + "N" + rand_dna(rng, 9)]
    K = 2
    want = [brute(strs, p, 20, K) + brute(strs, revcomp(p), 20, K, strand=1) for p in pats]
    both = fm.overlaps_mm(pats, min_overlap=20, mismatches=K, strands="both")
    check(both, pats, want)
    fwd = fm.overlaps_mm(pats, min_overlap=20, mismatches=K)
    rc = fm.overlaps_mm([revcomp(p) for p in pats], min_overlap=20, mismatches=K)
    n1 = m1 = 0
    for i in range(len(pats)):
        h = both.hits(i)
        assert np.array_equal(h[h["strand"] == 0], fwd.hits(i))
        minus = h[h["strand"] == 1].copy()
        n1 += len(minus)
        m1 += int((minus["flags"] >> 8 > 0).sum())
        minus["strand"] = 0
        assert np.array_equal(minus, rc.hits(i))
    assert n1 > 0 and m1 > 0


def test_longest_flag_is_the_host_reduction(api, synth):
    strs, _, _, fm = synth
    pats = strs + extra_queries(strs, 20)
    for strands in ("forward", "both"):
        full = fm.overlaps_mm(pats, min_overlap=20, mismatches=2, strands=strands)
        red = fm.overlaps_mm(pats, min_overlap=20, mismatches=2, strands=strands, longest=True)
        hits, offs = api.overlap_longest(full.all_hits, full.offsets)
        assert np.array_equal(red.offsets, offs) and np.array_equal(red.all_hits, hits)
        assert len(hits) < len(full.all_hits)
        assert fm.overlaps_mm_stats()["hits"] == len(hits)
        for i in (0, 17, len(strs) - 1):
            assert tuples(red, i) == longest_of(tuples(full, i))


def test_edge_queries(api, synth):
    strs, _, _, fm = synth
    rng = np.random.default_rng(5)
    ex = extra_queries(strs, 20)                             # lower case, N in the middle, N at the end, empty, short, ...
    whole = list(strs[4])
    whole[37] = "ACGT"[("ACGT".index(whole[37]) + 1) % 4]
    long_q = rand_dna(rng, max(len(s) for s in strs) + 50) + "".join(whole)
    p1024 = rand_dna(rng, 1024 - len(strs[8])) + strs[8]
    pats = ex + [long_q, p1024]
    K = 2
    want = [brute(strs, p, 20, K) for p in pats]
    res = fm.overlaps_mm(pats, min_overlap=20, mismatches=K)
    check(res, pats, want)
    assert want[0] and want[0] == brute(strs, strs[1], 20, K)                       # lower case
    mid = len(strs[3]) // 2
    assert any(fl >> 8 >= 1 and L > len(strs[3]) - mid for _, L, _, fl in want[1])   # a hit through the N
    assert want[2] and all(fl >> 8 >= 1 for _, _, _, fl in want[2])                  # N as the last base: always a mismatch
    assert want[3] == [] and want[4] == []                                           # empty, shorter than min_overlap
    assert any(fl & CONTAINS and not fl & WHOLE and fl >> 8 for _, _, _, fl in want[7])
    assert len(p1024) == 1024 and want[8]
    with pytest.raises(api.DebwtError) as e:
        fm.overlaps_mm(["A" + p1024], min_overlap=20, mismatches=1)
    assert e.value.code == -1


def test_small_buffers_do_not_change_results(api, synth, monkeypatch):
    strs, _, _, fm = synth
    pats = strs + extra_queries(strs, 20)
    names = ("DEBWT_FM_OVERLAP_ITEMS", "DEBWT_FM_OVERLAP_HITS", "DEBWT_FM_OVERLAP_BATCH")
    for n in names:
        monkeypatch.delenv(n, raising=False)
    ref = fm.overlaps_mm(pats, min_overlap=20, mismatches=2, strands="both")
    st0 = fm.overlaps_mm_stats()
    assert st0["batches"] == 1 and st0["retries"] == 0
    for items, hits, batch in (("1", None, None), (None, "64", None), (None, None, "50"), ("1", "64", "50")):
        for n, v in zip(names, (items, hits, batch)):
            monkeypatch.setenv(n, v) if v else monkeypatch.delenv(n, raising=False)
        got = fm.overlaps_mm(pats, min_overlap=20, mismatches=2, strands="both")
        st = fm.overlaps_mm_stats()
        assert same(got, ref), (items, hits, batch)
        assert st["hits"] == len(ref.all_hits) and st["runs"] == st0["runs"] and st["items"] == st0["items"]
        if items:
            assert st["retries"] > 0
        else:
            assert st["retries"] == 0
        if batch:
            assert st["batches"] == (len(pats) + 49) // 50
        else:
            assert st["batches"] == 1
        if hits:
            assert st["launches"] > len(ref.all_hits) // 64


def test_errors_and_capacity(api, synth):
    from debwt_amd import _lib
    strs, _, _, fm = synth
    pats = [p.encode() for p in strs[:40] + extra_queries(strs, 20)]
    buf = b"".join(pats)
    offs = np.zeros(len(pats) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in pats], out=offs[1:])
    L = _lib.lib()
    n = len(pats)
    hoff = np.zeros(n + 1, dtype=np.uint64)
    hp = ctypes.POINTER(_lib.DebwtFmOverlap)

    def call(o, min_overlap, K, permille, flags, cap, null=False):
        h = np.zeros(max(cap, 1), dtype=api._OVERLAP_DTYPE)
        rc = L.debwt_fm_overlaps_mm(fm._h, buf, api._p64(o), n, min_overlap, K, permille, flags, api._p64(hoff),
                                    None if null else h.ctypes.data_as(hp), cap)
        return rc, h

    assert call(offs, 20, 5, 0, 0, 10)[0] == -1 and b"max_mismatches" in L.debwt_fm_last_error(fm._h)
    assert call(offs, 20, 1, 1001, 0, 10)[0] == -1 and b"max_error_permille" in L.debwt_fm_last_error(fm._h)
    assert call(offs, 0, 1, 0, 0, 10)[0] == -1
    assert call(offs, 20, 1, 0, 4, 10)[0] == -1
    assert call(offs, 20, 1, 0, 8 | 1, 10)[0] == -1
    bad = offs.copy()
    bad[3] = bad[4] + 1
    assert call(bad, 20, 1, 0, 0, 10)[0] == -1
    with pytest.raises(ValueError):
        fm.overlaps_mm(["ACGT"], strands="reverse")
    for flags in (0, 1, 2, 3):
        res = fm.overlaps_mm([p.decode() for p in pats], min_overlap=20, mismatches=2, error_permille=60,
                             strands="both" if flags & 1 else "forward", longest=bool(flags & 2))
        total = len(res.all_hits)
        assert total > n
        hoff[:] = 0
        rc, _ = call(offs, 20, 2, 60, flags, 0, null=True)
        assert rc == -5 and np.array_equal(hoff, res.offsets)
        hoff[:] = 0
        rc, _ = call(offs, 20, 2, 60, flags, total - 1)
        assert rc == -5 and np.array_equal(hoff, res.offsets)
        rc, h = call(offs, 20, 2, 60, flags, total)
        assert rc == 0 and np.array_equal(hoff, res.offsets) and np.array_equal(h, res.all_hits)
    empty = fm.overlaps_mm([], min_overlap=20)
    assert len(empty) == 0 and len(empty.all_hits) == 0


def test_capacity_across_batches(api, synth, monkeypatch):
    """the count-only state is carried from batch to batch: the capacity runs out in the first batch, in the last one, or
    never, and the offsets are whole every time"""
    from debwt_amd import _lib
    _, _, qs, fm = synth
    pats = [p.encode() for p in qs]
    buf = b"".join(pats)
    offs = np.zeros(len(pats) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in pats], out=offs[1:])
    L = _lib.lib()
    n = len(pats)
    hoff = np.zeros(n + 1, dtype=np.uint64)

    def call(min_overlap, flags, cap, null=False):
        h = np.zeros(max(cap, 1), dtype=api._OVERLAP_DTYPE)
        hoff[:] = 77
        rc = L.debwt_fm_overlaps_mm(fm._h, buf, api._p64(offs), n, min_overlap, 2, 0, flags, api._p64(hoff),
                                    None if null else h.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmOverlap)), cap)
        return rc, h[:cap]

    for name in ("DEBWT_FM_OVERLAP_ITEMS", "DEBWT_FM_OVERLAP_HITS"):
        monkeypatch.delenv(name, raising=False)
    for flags in (0, 1, 2, 3):
        monkeypatch.delenv("DEBWT_FM_OVERLAP_BATCH", raising=False)
        res = fm.overlaps_mm(qs, min_overlap=20, mismatches=2, strands="both" if flags & 1 else "forward", longest=bool(flags & 2))
        total, first = len(res.all_hits), int(res.offsets[1])
        assert 1 <= first and int(res.offsets[50]) < total      # hits in the first batch of 50 patterns and behind it
        monkeypatch.setenv("DEBWT_FM_OVERLAP_BATCH", "50")
        for cap, null in ((0, True), (first - 1, False), (total - 1, False)):
            rc, _ = call(20, flags, cap, null)
            assert rc == -5 and np.array_equal(hoff, res.offsets), (flags, cap)
            assert fm.overlaps_mm_stats()["batches"] == (n + 49) // 50 > 3 and fm.overlaps_mm_stats()["hits"] == total
        rc, h = call(20, flags, total)
        assert rc == 0 and np.array_equal(hoff, res.offsets) and np.array_equal(h, res.all_hits)
        assert fm.overlaps_mm_stats()["batches"] == (n + 49) // 50
    # No pattern has a hit, no array is given: without LONGEST nothing is missing and the call succeeds; with LONGEST a
    # NULL array never fits, so the call asks for room for 0 hits.  The two branches have differed since the call came
    # in; the difference is pinned as recorded on the parent of the fold, not repaired.
    longer = max(len(p) for p in pats) + 1
    for flags, want in ((0, 0), (1, 0), (2, -5), (3, -5)):
        rc, _ = call(longer, flags, 0, null=True)
        assert rc == want and not hoff.any(), flags
        assert fm.overlaps_mm_stats()["hits"] == 0 and fm.overlaps_mm_stats()["batches"] == (n + 49) // 50


# Every field of overlaps_mm_stats() that is no time, for the 165 queries at min_overlap 20 with 2 mismatches on both
# strands, by (longest, limits); limits True sets DEBWT_FM_OVERLAP_ITEMS=1, DEBWT_FM_OVERLAP_HITS=64 and
# DEBWT_FM_OVERLAP_BATCH=50.  Recorded on an MI355X at ad9150c, the commit before the exact and the mismatch call shared
# one host path, in two runs that agreed in every field but wave_steps (604096 and 604992 without limits: the order in
# which a level's children land decides which items share a wave), which is therefore left out.  A difference in any
# other field means a launch, a batch or a buffer changed.
_WALK = {"patterns": 165, "runs": 1424, "steps": 177008, "line_reads": 208341, "items": [330, 6655, 48152, 0, 0]}
PINNED = {
    (False, False): dict(_WALK, batches=1, launches=4, retries=0, hits=1455, scratch_bytes=536928368),
    (True, False): dict(_WALK, batches=1, launches=4, retries=0, hits=1339, scratch_bytes=536928368),
    (False, True): dict(_WALK, batches=4, launches=90, retries=6, hits=1455, scratch_bytes=278904),
    (True, True): dict(_WALK, batches=4, launches=90, retries=6, hits=1339, scratch_bytes=278904),
}


@pytest.mark.parametrize("limits", [False, True])
def test_stats_are_pinned(api, synth, monkeypatch, limits):
    strs, _, pats, fm = synth
    assert len(pats) == 165
    for name, v in (("DEBWT_FM_OVERLAP_ITEMS", "1"), ("DEBWT_FM_OVERLAP_HITS", "64"), ("DEBWT_FM_OVERLAP_BATCH", "50")):
        monkeypatch.setenv(name, v) if limits else monkeypatch.delenv(name, raising=False)
    got = {}
    for longest in (False, True):
        fm.overlaps_mm(pats, min_overlap=20, mismatches=2, strands="both", longest=longest)
        got[longest, limits] = {k: v for k, v in fm.overlaps_mm_stats().items() if not k.startswith("ms_") and k != "wave_steps"}
        print("PINNED[%r, %r] = %r" % (longest, limits, got[longest, limits]))
    assert got == {k: v for k, v in PINNED.items() if k[1] == limits}


def test_index_from_files(api):
    entry = entry_named("shared_ends_duplicates")
    recs = golden_records(entry)
    strs = ["".join("ACGT"[c] for c in np.asarray(r).tolist()) for r in recs]
    text, _ = text_of(recs)
    words, hrows, drow = golden_outputs(entry)
    own = index_of(api, recs, s=4)
    opened = api.FMIndex.open(words, len(text), hrows, drow, own.samples(), sa_sample=4)     # no text is ever attached
    rng = np.random.default_rng(13)
    pats = []
    for s in strs:
        t = list(rand_dna(rng, 25) + s[:30])
        t[40] = "ACGT"[("ACGT".index(t[40]) + 1) % 4]
        pats.append("".join(t))
    a = own.overlaps_mm(pats, min_overlap=8, mismatches=2, strands="both")
    b = opened.overlaps_mm(pats, min_overlap=8, mismatches=2, strands="both")
    assert len(a.all_hits) > len(pats) and int(a.mismatches().max()) >= 1
    assert same(a, b)
    check(b, pats, [brute(strs, p, 8, 2) + brute(strs, revcomp(p), 8, 2, strand=1) for p in pats])
    own.close(); opened.close()


def test_stats(api, synth):
    strs, _, pats, fm = synth
    for K, strands in ((0, "forward"), (2, "both"), (4, "forward")):
        res = fm.overlaps_mm(pats, min_overlap=20, mismatches=K, strands=strands)
        st = fm.overlaps_mm_stats()
        assert st["patterns"] == len(pats) and st["batches"] == 1
        assert st["items"][0] == len(pats) * (2 if strands == "both" else 1)
        assert all(st["items"][l] > 0 for l in range(K + 1)) and all(st["items"][l] == 0 for l in range(K + 1, 5))
        assert st["hits"] == len(res.all_hits) and st["runs"] <= st["hits"]
        assert 0 < st["steps"] <= st["wave_steps"] and st["line_reads"] >= st["steps"]
        assert st["ms_kernel"] > 0 and st["ms_wall"] > 0 and st["scratch_bytes"] > 0 and st["launches"] >= K + 2


def test_golden_reads(api):
    recs = golden_records(entry_named("reads_20000"))
    strs = ["".join("ACGT"[c] for c in np.asarray(r).tolist()) for r in recs]
    sample = strs[::40]                                      # the reference costs 20,000 x m^2 / 2 comparisons per query:
    pats = [s for s in sample if len(s) <= 160][:96] + [s for s in sample if len(s) > 300][:4]   # mostly short, four long
    assert len(pats) == 100
    want = [brute(strs, p, 30, 1) for p in pats]
    assert sum(1 for w in want for h in w if h[3] >> 8) > 0
    fm = index_of(api, recs)
    check(fm.overlaps_mm(pats, min_overlap=30, mismatches=1), pats, want)
    fm.close()
