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
