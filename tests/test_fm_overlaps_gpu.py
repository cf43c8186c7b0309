"""Suffix-prefix overlaps (debwt_fm_overlaps, FMIndex.overlaps) against the reference of overlap_ref.py: the whole ordered
hit list of every query, flags included, compared exactly -- on a synthetic read set with duplicates, contained and
periodic records, on goldens (one record, special branches, shared ends) and on 20,000 reads; both strands, the longest
reduction, batches cut by tiny limits, errors and the capacity protocol, an index from files, statistics."""
import ctypes

import numpy as np
import pytest

from conftest import golden_outputs, golden_records
from overlap_ref import CONTAINS, WHOLE, Ref, codes, extra_queries, longest_of, rand_dna, revcomp, synthetic_reads
from test_fm_index_gpu import text_of
from test_fm_search_gpu import entry_named, index_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def rec_strings(recs):
    return ["".join("ACGT"[c] for c in np.asarray(r).tolist()) for r in recs]


@pytest.fixture(scope="module")
def synth(api):
    """(record strings, their index): built once, queried by every test below and never changed"""
    strs = synthetic_reads()
    assert min(len(s) for s in strs) >= 40
    fm = index_of(api, codes(strs), s=4)
    yield strs, fm
    fm.close()


def tuples(res, i):
    return [tuple(int(x) for x in h) for h in res.hits(i).tolist()]


def check(res, pats, want):
    assert len(res) == len(pats)
    for i, p in enumerate(pats):
        assert tuples(res, i) == want[i], (i, p)
    assert int(res.count().sum()) == sum(len(w) for w in want) == len(res.all_hits)


def test_reference_has_every_kind_of_hit():
    """at min_overlap 20 the reference alone holds each category the GPU comparison is meant to cover"""
    strs = synthetic_reads()
    R = Ref(strs, 20)
    last = len(strs) - 1
    kinds = set()
    for i, p in enumerate(strs):
        hits = R.hits(p)
        pairs = [h[0] for h in hits]
        for j, L, _, fl in hits:
            for kind, holds in (("contains", fl & CONTAINS), ("whole", fl & WHOLE), ("neither flag", fl == 0),
                                ("both flags, another record", fl == (CONTAINS | WHOLE) and j != i),
                                ("record 0", j == 0), ("last record", j == last)):
                if holds:
                    kinds.add(kind)
        if len(set(pairs)) < len(pairs):
            kinds.add("one record at several lengths")
    assert kinds == {"contains", "whole", "both flags, another record", "record 0", "last record", "neither flag",
                     "one record at several lengths"}
    long_q = extra_queries(strs, 20)[5]
    assert any(fl == CONTAINS for _, _, _, fl in R.hits(long_q))     # CONTAINS without WHOLE
    n_end = extra_queries(strs, 20)[2]
    assert R.hits(n_end) == [] and R.hits(extra_queries(strs, 20)[1]) != []


@pytest.mark.parametrize("min_overlap", [1, 20, 41])
def test_synthetic_read_set(api, synth, min_overlap):
    strs, fm = synth
    R = Ref(strs, min_overlap)
    pats = strs + extra_queries(strs, min_overlap)
    want = [R.hits(p) for p in pats]
    res = fm.overlaps(pats, min_overlap=min_overlap)
    check(res, pats, want)
    st = fm.overlaps_stats()
    assert st["hits"] == len(res.all_hits) and st["patterns"] == len(pats) and st["batches"] == 1
    assert 0 < st["steps"] <= st["wave_steps"] and st["line_reads"] >= st["steps"] and st["runs"] <= st["hits"]
    assert st["launches"] >= 3 and st["scratch_bytes"] > 0 and st["ms_kernel"] > 0 and st["ms_wall"] > 0


def test_both_strands(api, synth):
    strs, fm = synth
    R = Ref(strs, 20)
    rng = np.random.default_rng(7)
    pats = strs[::3] + [revcomp(s) for s in strs[1::5]] + extra_queries(strs, 20)
    pats += [revcomp(strs[6])[:50] + rand_dna(rng, 30), revcomp(strs[7][:33]).lower() + "N" + rand_dna(rng, 9)]
    both = fm.overlaps(pats, min_overlap=20, strands="both")
    check(both, pats, [R.both(p) for p in pats])
    fwd = fm.overlaps(pats, min_overlap=20)
    rc = fm.overlaps([revcomp(p) for p in pats], min_overlap=20)
    n1 = 0
    for i in range(len(pats)):
        h = both.hits(i)
        assert np.array_equal(h[h["strand"] == 0], fwd.hits(i))
        minus = h[h["strand"] == 1].copy()
        n1 += len(minus)
        minus["strand"] = 0
        assert np.array_equal(minus, rc.hits(i))
    assert n1 > 0


def test_longest_flag_is_the_host_reduction(api, synth):
    strs, fm = synth
    pats = strs + extra_queries(strs, 1)
    for strands in ("forward", "both"):
        full = fm.overlaps(pats, min_overlap=1, strands=strands)
        red = fm.overlaps(pats, min_overlap=1, strands=strands, longest=True)
        hits, offs = api.overlap_longest(full.all_hits, full.offsets)
        assert np.array_equal(red.offsets, offs) and np.array_equal(red.all_hits, hits)
        assert len(hits) < len(full.all_hits)
        assert fm.overlaps_stats()["hits"] == len(hits)
        for i in (0, 17, len(strs) - 1):
            assert tuples(red, i) == longest_of(tuples(full, i))


def test_batches_do_not_change_results(api, synth, monkeypatch):
    strs, fm = synth
    pats = strs + extra_queries(strs, 1)
    monkeypatch.delenv("DEBWT_FM_OVERLAP_SLOTS", raising=False)
    monkeypatch.delenv("DEBWT_FM_OVERLAP_HITS", raising=False)
    ref = {(L, lg): fm.overlaps(pats, min_overlap=L, strands="both", longest=lg) for L, lg in ((1, False), (20, True))}
    assert fm.overlaps_stats()["batches"] == 1
    for slots, hits in (("64", None), (None, "64"), ("64", "64")):
        for name, v in (("DEBWT_FM_OVERLAP_SLOTS", slots), ("DEBWT_FM_OVERLAP_HITS", hits)):
            monkeypatch.setenv(name, v) if v else monkeypatch.delenv(name, raising=False)
        for (L, lg), want in ref.items():
            got = fm.overlaps(pats, min_overlap=L, strands="both", longest=lg)
            st = fm.overlaps_stats()
            assert np.array_equal(got.offsets, want.offsets) and np.array_equal(got.all_hits, want.all_hits), (slots, hits, L, lg)
            assert st["hits"] == len(want.all_hits)
            if slots:
                assert st["batches"] > 3
            elif L == 1:
                assert st["batches"] == 1 and st["launches"] > 3          # one batch, expanded 64 hits at a launch


@pytest.mark.parametrize("name,min_overlap", [("shared_ends_duplicates", 8), ("special_branches", 8), ("single_record", 8),
                                              ("shared_ends_duplicates", 20), ("reads_20000", 30)])
def test_goldens(api, name, min_overlap):
    recs = golden_records(entry_named(name))
    strs = rec_strings(recs)
    R = Ref(strs, min_overlap)
    rng = np.random.default_rng(11)
    if name == "reads_20000":
        pats = strs[::10]
    else:
        pats = [s for s in strs if len(s) <= 4000] + [rand_dna(rng, 40) + s[:int(rng.integers(8, min(len(s), 90) + 1))] for s in strs]
        pats += [strs[0][:50], rand_dna(rng, 30) + strs[-1][:9] + "N", ""]
    want = [R.both(p) for p in pats]
    assert sum(len(w) for w in want) > 0
    fm = index_of(api, recs)
    check(fm.overlaps(pats, min_overlap=min_overlap, strands="both"), pats, want)
    fm.close()


def test_errors_and_capacity(api, synth):
    from debwt_amd import _lib
    strs, fm = synth
    pats = [p.encode() for p in strs[:40] + extra_queries(strs, 20)]
    buf = b"".join(pats)
    offs = np.zeros(len(pats) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in pats], out=offs[1:])
    L = _lib.lib()
    n = len(pats)
    hoff = np.zeros(n + 1, dtype=np.uint64)
    hp = ctypes.POINTER(_lib.DebwtFmOverlap)

    def call(o, min_overlap, flags, cap, null=False):
        h = np.zeros(max(cap, 1), dtype=api._OVERLAP_DTYPE)
        rc = L.debwt_fm_overlaps(fm._h, buf, api._p64(o), n, min_overlap, flags, api._p64(hoff),
                                 None if null else h.ctypes.data_as(hp), cap)
        return rc, h

    assert call(offs, 0, 0, 10)[0] == -1
    assert call(offs, 20, 4, 10)[0] == -1
    assert call(offs, 20, 8 | 1, 10)[0] == -1
    bad = offs.copy()
    bad[3] = bad[4] + 1
    assert call(bad, 20, 0, 10)[0] == -1
    with pytest.raises(api.DebwtError) as e:
        fm.overlaps(["ACGT"], min_overlap=0)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        fm.overlaps(["ACGT"], strands="reverse")
    for flags in (0, 1, 2, 3):
        res = fm.overlaps(pats, min_overlap=20, strands="both" if flags & 1 else "forward", longest=bool(flags & 2))
        total = len(res.all_hits)
        assert total > n
        hoff[:] = 0
        rc, _ = call(offs, 20, flags, 0, null=True)
        assert rc == -5 and np.array_equal(hoff, res.offsets)
        hoff[:] = 0
        rc, _ = call(offs, 20, flags, total - 1)
        assert rc == -5 and np.array_equal(hoff, res.offsets)
        rc, h = call(offs, 20, flags, total)
        assert rc == 0 and np.array_equal(hoff, res.offsets) and np.array_equal(h, res.all_hits)
    empty = fm.overlaps([], min_overlap=20)
    assert len(empty) == 0 and len(empty.all_hits) == 0
    assert tuples(fm.overlaps([strs[0]], min_overlap=len(strs[0]) + 1), 0) == []


def test_capacity_across_batches(api, synth, monkeypatch):
    """the count-only state is carried from batch to batch: the capacity runs out in the first batch, in the last one, or
    never, and the offsets are whole every time"""
    from debwt_amd import _lib
    strs, fm = synth
    pats = [p.encode() for p in strs[:40] + extra_queries(strs, 20)]
    buf = b"".join(pats)
    offs = np.zeros(len(pats) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in pats], out=offs[1:])
    L = _lib.lib()
    n = len(pats)
    hoff = np.zeros(n + 1, dtype=np.uint64)

    def call(min_overlap, flags, cap, null=False):
        h = np.zeros(max(cap, 1), dtype=api._OVERLAP_DTYPE)
        hoff[:] = 77
        rc = L.debwt_fm_overlaps(fm._h, buf, api._p64(offs), n, min_overlap, flags, api._p64(hoff),
                                 None if null else h.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmOverlap)), cap)
        return rc, h[:cap]

    monkeypatch.delenv("DEBWT_FM_OVERLAP_HITS", raising=False)
    for flags in (0, 1, 2, 3):
        monkeypatch.delenv("DEBWT_FM_OVERLAP_SLOTS", raising=False)
        res = fm.overlaps(pats, min_overlap=20, strands="both" if flags & 1 else "forward", longest=bool(flags & 2))
        total, first = len(res.all_hits), int(res.offsets[1])
        assert 1 <= first < total                               # pattern 0 is in the first batch whatever the limits
        monkeypatch.setenv("DEBWT_FM_OVERLAP_SLOTS", "64")
        for cap, null in ((0, True), (first - 1, False), (total - 1, False)):
            rc, _ = call(20, flags, cap, null)
            assert rc == -5 and np.array_equal(hoff, res.offsets), (flags, cap)
            assert fm.overlaps_stats()["batches"] > 3 and fm.overlaps_stats()["hits"] == total
        rc, h = call(20, flags, total)
        assert rc == 0 and np.array_equal(hoff, res.offsets) and np.array_equal(h, res.all_hits)
        assert fm.overlaps_stats()["batches"] > 3
    # No pattern has a hit, no array is given: without LONGEST nothing is missing and the call succeeds; with LONGEST a
    # NULL array never fits, so the call asks for room for 0 hits.  The two branches have differed since the call came
    # in; the difference is pinned as recorded on the parent of the fold, not repaired.
    longer = max(len(p) for p in pats) + 1
    for flags, want in ((0, 0), (1, 0), (2, -5), (3, -5)):
        rc, _ = call(longer, flags, 0, null=True)
        assert rc == want and not hoff.any(), flags
        assert fm.overlaps_stats()["hits"] == 0 and fm.overlaps_stats()["batches"] >= 1


# Every field of overlaps_stats() that is no time, for strs + extra_queries(strs, L) on both strands, by (L, longest,
# limits); limits "64" sets DEBWT_FM_OVERLAP_SLOTS and DEBWT_FM_OVERLAP_HITS.  Recorded on an MI355X at ad9150c, the commit
# before the exact and the mismatch call shared one host path, twice with equal values: they are sums and counts, and the
# batches depend on the input and the two limits alone.  A difference means a launch, a batch or a buffer changed.
_WALK = {"patterns": 443, "steps": 38107, "line_reads": 42607}
PINNED = {
    (1, False, None): dict(_WALK, batches=1, launches=3, runs=8712, hits=133999, wave_steps=60416, scratch_bytes=3531208),
    (20, True, None): dict(_WALK, batches=1, launches=3, runs=3997, hits=3960, wave_steps=60416, scratch_bytes=1072912),
    (1, False, "64"): dict(_WALK, batches=442, launches=3165, runs=8712, hits=133999, wave_steps=2249152, scratch_bytes=18536),
    (20, True, "64"): dict(_WALK, batches=442, launches=1320, runs=3997, hits=3960, wave_steps=2249152, scratch_bytes=16784),
}


@pytest.mark.parametrize("limits", [None, "64"])
def test_stats_are_pinned(api, synth, monkeypatch, limits):
    strs, fm = synth
    for name in ("DEBWT_FM_OVERLAP_SLOTS", "DEBWT_FM_OVERLAP_HITS"):
        monkeypatch.setenv(name, limits) if limits else monkeypatch.delenv(name, raising=False)
    got = {}
    for L, longest in ((1, False), (20, True)):
        res = fm.overlaps(strs + extra_queries(strs, L), min_overlap=L, strands="both", longest=longest)
        assert not (res.all_hits["flags"] & np.uint32(~3 & 0xFFFFFFFF)).any()   # no mismatch bits from the shared expansion
        got[L, longest, limits] = {k: v for k, v in fm.overlaps_stats().items() if not k.startswith("ms_")}
        print("PINNED[%r, %r, %r] = %r" % (L, longest, limits, got[L, longest, limits]))
    assert got == {k: v for k, v in PINNED.items() if k[2] == limits}


def test_index_from_files(api):
    entry = entry_named("shared_ends_duplicates")
    recs = golden_records(entry)
    strs = rec_strings(recs)
    text, _ = text_of(recs)
    words, hrows, drow = golden_outputs(entry)
    own = index_of(api, recs, s=4)
    opened = api.FMIndex.open(words, len(text), hrows, drow, own.samples(), sa_sample=4)     # no text is ever attached
    rng = np.random.default_rng(13)
    pats = strs + [rand_dna(rng, 25) + s[:30] for s in strs]
    before = opened.info()["device_bytes"]
    a = own.overlaps(pats, min_overlap=8, strands="both")
    b = opened.overlaps(pats, min_overlap=8, strands="both")
    assert len(a.all_hits) > len(pats)
    assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.all_hits, b.all_hits)
    after = opened.info()["device_bytes"]
    assert after >= before + 8 * len(recs)                    # the record table, 8 bytes per record
    c = opened.overlaps(pats, min_overlap=8, strands="both")
    assert opened.info()["device_bytes"] == after and np.array_equal(c.all_hits, b.all_hits)
    own.close(); opened.close()
