"""Alignment against a text window (debwt_fm_align_window): every field of the alignment and the whole CIGAR against
fm_path_ref.path_ref, the one alignment include/debwt_hip.h documents, over the cells of the window clipped to its record.
path_ref takes allowed cells as a band around anchors; `window_ref` gives every query row its own anchor so that the band
is the window itself (the columns [lo, hi) in every row), which keeps the reference's rows as narrow as the window; one
test shows that the single anchor (0, wbeg) with w >= m + window length is the same alignment."""
import ctypes
import re

import numpy as np
import pytest

from fm_path_ref import path_ref
from test_fm_extend_contract_gpu import COLLECTIONS, result, world  # noqa: F401  (world: a fixture)
from test_fm_extend_chain_gpu import ChainRef
from test_fm_extend_gpu import index_with_text, mutated_reads
from test_fm_mems_gpu import revcomp
from test_fm_search_gpu import index_of

pytestmark = pytest.mark.gpu
SC_A, SC_B = (1, 4, 6, 1), (2, 3, 0, 2)
MS = [1, 2, 63, 64, 65, 128, 150]
LS = [1, 2, 63, 64, 65, 127, 128, 129, 400]


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def window_ref(R, p, job, sc, info=None):
    """path_ref over the cells 0 <= i < m, max(rs, wbeg) <= t < min(re, wend) of job (pattern, strand, record, wbeg, wend)"""
    _, strand, rec, wbeg, wend = job
    q = R.query(p, strand)
    lo, hi = max(R.rs[rec], wbeg), min(R.re[rec], wend)
    if lo >= hi:
        return (0, 0, 0, 0, 0, 0, [])
    half = (hi - lo) // 2
    anchors = [(i, lo + half - i) for i in range(len(q))]      # row i is centred on text position lo + half
    return path_ref(q, R.text, lo, hi, anchors, half + 1, sc, info)


def check(R, fm, pats, jobs, sc, refs=None):
    refs = [window_ref(R, pats[j[0]], j, sc) for j in jobs] if refs is None else refs
    res = fm.align_window(pats, jobs, scoring=sc)
    assert len(res) == len(jobs)
    for k, want in enumerate(refs):
        assert result(res, k) == want, (jobs[k], pats[jobs[k][0]], sc)
    assert int(res.offsets[-1]) == len(res.cigars) == sum(len(r[6]) for r in refs)
    so = fm.align_window(pats, jobs, scoring=sc, cigar=False)
    for k, want in enumerate(refs):
        assert (int(so.score[k]), int(so.qbeg[k]), int(so.qend[k]), int(so.tbeg[k]), int(so.tend[k]), int(so.edits[k])) == \
               (want[0], 0, want[2], 0, want[4], 0)
    return res


def edited(rng, s, nedit, with_n):
    s = list(s)
    for _ in range(nedit):
        kind, j = int(rng.integers(0, 3)), int(rng.integers(0, len(s)))
        if kind == 0:
            s[j] = "ACGT"[int(rng.integers(0, 4))]
        elif kind == 1:
            s.insert(j, "ACGT"[int(rng.integers(0, 4))])
        elif len(s) > 2:
            del s[j]
    if with_n and len(s) > 1:
        s[int(rng.integers(0, len(s)))] = "N"
    return "".join(s)


def cut(rng, R, rec, start, m, nedit, with_n, strand):
    """a query of exactly m bases cut from record rec at `start` (clipped to the record), edited, as given on `strand`"""
    r = R.strs[rec]
    a = min(max(start - R.rs[rec], 0), max(len(r) - m, 0))
    s = edited(rng, r[a:a + m], nedit, with_n) if m > 1 else r[a:a + 1]
    s = (s + "".join("ACGT"[int(x)] for x in rng.integers(0, 4, m)))[:m]
    return revcomp(s) if strand else s


@pytest.fixture(scope="module")
def plain(api):
    """random records: one long enough for the widest window, short neighbours on both sides"""
    rng = np.random.default_rng(77)
    recs = [rng.integers(0, 4, size=n).astype(np.uint8) for n in (300, 17000, 90, 700)]
    fm = index_with_text(api, recs)
    yield ChainRef(recs), fm
    fm.close()


@pytest.mark.parametrize("m", MS)
def test_shapes_at_strip_and_lane_edges(plain, m):
    """every m with every window length; each (m, L) on strand 0 under one scoring and on strand 1 under the other, the
    pairing alternating, so that both strands meet both scorings at every m"""
    R, fm = plain
    rng = np.random.default_rng(1000 + m)
    by_sc = {SC_A: ([], []), SC_B: ([], [])}
    for n, L in enumerate(LS):
        for strand in (0, 1):
            sc = SC_A if (n + strand) % 2 == 0 else SC_B
            pats, jobs = by_sc[sc]
            rec = 1 if n % 3 else 3
            wbeg = R.rs[rec] + int(rng.integers(0, len(R.strs[rec]) - L + 1))
            start = wbeg + int(rng.integers(-(m // 2), max(L - m // 2, 1)))
            pats.append(cut(rng, R, rec, start, m, int(rng.integers(0, 5)), n % 2 == 1, strand))
            jobs.append((len(pats) - 1, strand, rec, wbeg, wbeg + L))
    positive = 0
    for sc, (pats, jobs) in by_sc.items():
        assert all(len(p) == m for p in pats)
        res = check(R, fm, pats, jobs, sc)
        positive += int((res.score > 0).sum())
    assert positive >= len(LS)


def test_one_anchor_and_a_wide_band_is_the_same_reference(plain):
    R, _ = plain
    rng = np.random.default_rng(3)
    for m, L, strand in ((20, 70, 0), (65, 30, 1), (40, 129, 1)):
        wbeg = R.rs[3] + 100
        p = cut(rng, R, 3, wbeg + 5, m, 3, True, strand)
        job = (0, strand, 3, wbeg, wbeg + L)
        a = path_ref(R.query(p, strand), R.text, max(R.rs[3], wbeg), min(R.re[3], wbeg + L), [(0, wbeg)], m + L, SC_A)
        assert a == window_ref(R, p, job, SC_A) and a[0] > 0


def test_largest_hand_over_and_largest_strip_count(plain):
    """m = 4096 over one strip of 64 columns next to a second strip (the hand-over buffer at its 32 KiB), and 33 rows over
    the 256 strips of the widest window"""
    R, fm = plain
    rng = np.random.default_rng(9)
    rs = R.rs[1]
    tall = cut(rng, R, 1, rs + 2000, 4096, 4, True, 0)
    wide = cut(rng, R, 1, rs + 9000, 33, 2, False, 1)
    pats = [tall, wide]
    jobs = [(0, 0, 1, rs + 3000, rs + 3064), (0, 0, 1, rs + 3000, rs + 3065), (1, 1, 1, rs + 300, rs + 300 + 16384)]
    res = check(R, fm, pats, jobs, SC_A)
    assert int(res.score[0]) > 0 and int(res.score[1]) > 0 and int(res.score[2]) > 0
    st = fm.extend_stats()
    assert st["jobs"] == 3 and st["cells"] == 4096 * 64 + 4096 * 65 + 33 * 16384
    assert st["wave_steps"] == (4096 + 63) + (4096 + 63 + 4096) + (255 * (33 + 63) + 33 + 63)
    assert 0 < st["cells"] <= 64 * st["wave_steps"]


def test_clipping(plain):
    R, fm = plain
    rng = np.random.default_rng(21)
    rs, re = R.rs[2], R.re[2]                                     # the record of 90 bases between two others
    p = cut(rng, R, 2, rs, 50, 2, False, 0)
    p2 = cut(rng, R, 2, re - 40, 40, 1, False, 1)
    pats = [p, p2]
    jobs = [(0, 0, 2, rs - 120, rs + 70), (0, 0, 2, rs, rs + 70),           # reaching before the start = clipped
            (1, 1, 2, re - 60, re + 200), (1, 1, 2, re - 60, re),           # reaching past the end = clipped
            (0, 0, 2, rs - 8000, re + 8000), (0, 0, 2, rs, re),             # far over both ends = the record
            (0, 0, 2, R.rs[1] + 10, R.rs[1] + 500), (0, 0, 2, R.rs[3], R.rs[3] + 100),   # wholly in a neighbour: score 0
            (0, 0, 2, rs + 10, rs + 10), (1, 1, 2, re, re), (0, 0, 2, re, re + 1),       # wbeg == wend; the separator
            (1, 1, 3, R.re[3] - 20, R.re[3] + 5000), (1, 0, 0, 0, 10)]       # the last record's end, the text's start
    res = check(R, fm, pats, jobs, SC_A)
    for a, b in ((0, 1), (2, 3), (4, 5)):
        assert result(res, a) == result(res, b) and int(res.score[a]) > 0
    for k in (6, 7, 8, 9, 10):
        assert result(res, k) == (0, 0, 0, 0, 0, 0, [])


@pytest.fixture(scope="module")
def tie_cases(world):
    """reads of the two tie-rich collections (homopolymer and tandem-repeat records, records that share their ends), each
    against a window of up to 260 columns around its origin, with the references and what they met"""
    out = []
    for ci, name in enumerate(COLLECTIONS):
        R, _ = world(name)
        rng = np.random.default_rng(40 + ci)
        reads = mutated_reads(R, rng, 8, lo=20, hi=70)
        for n, (p, strand, rec, pos, _) in enumerate(reads):
            wbeg = max(R.rs[rec], pos - int(rng.integers(0, 120)))
            job = (n, strand, rec, wbeg, min(R.re[rec], wbeg + 260))
            for sc in ((SC_A, SC_B), ((1, 1, 0, 1), (255, 255, 255, 255)))[n % 2]:
                info = {}
                out.append((name, p, job, sc, window_ref(R, p, job, sc, info), info))
        # a third of the collection's longest run of one base, against the run and 40 columns on either side: every
        # placement inside the run scores the same, so the end cell is decided by the rule
        runs = [(max(re.finditer(r"A+|C+|G+|T+", s), key=lambda x: len(x.group())), k) for k, s in enumerate(R.strs)]
        run, rec = max(runs, key=lambda x: len(x[0].group()))
        p = run.group()[:len(run.group()) // 3]
        job = (len(reads), ci, rec, max(R.rs[rec], R.rs[rec] + run.start() - 40), min(R.re[rec], R.rs[rec] + run.end() + 40))
        for sc in (SC_A, (255, 255, 255, 255)):
            info = {}
            out.append((name, revcomp(p) if ci else p, job, sc, window_ref(R, revcomp(p) if ci else p, job, sc, info), info))
    return out


def test_ties(world, tie_cases):
    assert sum(i["end_ties"] > 0 for *_, i in tie_cases) > 0 and sum(i["ties"] > 0 for *_, i in tie_cases) > 0
    assert any(sc == (255, 255, 255, 255) and i["ties"] for _, _, _, sc, _, i in tie_cases)
    for name in COLLECTIONS:
        R, fm = world(name)
        for sc in sorted({c[3] for c in tie_cases}):
            mine = [c for c in tie_cases if c[0] == name and c[3] == sc]
            pats = [c[1] for c in mine]
            jobs = [(k,) + c[2][1:] for k, c in enumerate(mine)]
            check(R, fm, pats, jobs, sc, refs=[c[4] for c in mine])


@pytest.fixture(scope="module")
def short_records(api):
    """records of 33..64 bases, random and repetitive"""
    rng = np.random.default_rng(5)
    recs = [rng.integers(0, 4, size=n).astype(np.uint8) for n in (33, 64, 47, 63, 40, 58)]
    recs += [np.tile(np.array([0, 1], np.uint8), 32), np.concatenate([rng.integers(0, 4, 20), np.zeros(30, np.int64)]).astype(np.uint8),
             np.tile(np.array([2, 3, 3], np.uint8), 15)[:41]]
    fm = index_with_text(api, recs)
    yield ChainRef(recs), fm
    fm.close()


def test_bit_for_bit_bridge_to_the_banded_kernel(short_records):
    """a record of at most 64 bases, a query of at most 64: the window that is the record and the band of 63 diagonals
    around diag = rs + (len - m) / 2 allow the same cells, so both kernels must return the same bits"""
    R, fm = short_records
    rng = np.random.default_rng(6)
    pats, wjobs, xjobs = [], [], []
    for rec, r in enumerate(R.strs):
        for m in (1, 17, 33, 63, 64):
            strand = (rec + m) % 2
            a = int(rng.integers(0, max(len(r) - m, 0) + 1))
            s = edited(rng, r[a:a + m], int(rng.integers(0, 4)), m % 3 == 0) if m > 1 else r[a]
            s = (s + r + r)[:m]
            pats.append(revcomp(s) if strand else s)
            wjobs.append((len(pats) - 1, strand, rec, R.rs[rec], R.re[rec]))
            xjobs.append((len(pats) - 1, strand, R.rs[rec] + (len(r) - m) // 2, rec))
    for sc in (SC_A, SC_B, (255, 255, 255, 255)):
        a = fm.align_window(pats, wjobs, scoring=sc)
        b = fm.extend(pats, xjobs, scoring=sc, band=63)
        assert a.aln.tobytes() == b.aln.tobytes() and (a.score > 0).sum() > len(pats) // 2
        assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.cigars, b.cigars)
    check(R, fm, pats, wjobs, SC_A)


def some_jobs(R, rng, count=24):
    pats, jobs = [], []
    for n in range(count):
        m, L = int(rng.integers(1, 120)), int(rng.integers(1, 300))
        wbeg = R.rs[1] + int(rng.integers(0, 15000))
        pats.append(cut(rng, R, 1, wbeg + int(rng.integers(0, L)), m, int(rng.integers(0, 4)), False, n % 2))
        jobs.append((n, n % 2, 1, wbeg, wbeg + L))
    return pats, jobs


def test_batching_does_not_change_the_result(plain, monkeypatch):
    R, fm = plain
    pats, jobs = some_jobs(R, np.random.default_rng(11))
    full = fm.align_window(pats, jobs, scoring=SC_B)
    one = fm.extend_stats()
    assert one["batches"] == 1 and one["launches"] == 3 and 0 < one["cells"] <= 64 * one["wave_steps"]
    assert one["cells"] == sum(len(pats[j[0]]) * (j[4] - j[3]) for j in jobs)
    monkeypatch.setenv("DEBWT_FM_EXTEND_BYTES", "4096")
    cut_up = fm.align_window(pats, jobs, scoring=SC_B)
    many = fm.extend_stats()
    assert many["batches"] > len(jobs) // 2 and many["cells"] == one["cells"] and many["wave_steps"] == one["wave_steps"]
    assert full.aln.tobytes() == cut_up.aln.tobytes()
    assert np.array_equal(full.offsets, cut_up.offsets) and np.array_equal(full.cigars, cut_up.cigars)
    so = fm.align_window(pats, jobs, scoring=SC_B, cigar=False)
    assert np.array_equal(so.score, full.score) and np.array_equal(so.qend, full.qend) and np.array_equal(so.tend, full.tend)
    assert fm.extend_stats()["scratch_bytes"] == 0
    for k in (0, 5, 17):                                        # spot checks against the reference
        assert result(full, k) == window_ref(R, pats[k], jobs[k], SC_B)


def raw_call(api, fm, pats, jobs, sc, capacity, with_offsets=True):
    from debwt_amd import _lib
    buf, offs = api._patterns(pats)
    ja = (_lib.DebwtFmWindowJob * max(len(jobs), 1))()
    for k, (p, s, r, b, e) in enumerate(jobs):
        ja[k].pattern, ja[k].strand, ja[k].record, ja[k].wbeg, ja[k].wend = p, s, r, b, e
    s = _lib.DebwtFmScoring(*sc)
    out = np.zeros(max(len(jobs), 1), dtype=api._ALN_DTYPE)
    coff = np.full(len(jobs) + 1, 2 ** 64 - 1, dtype=np.uint64)
    cg = np.zeros(max(capacity, 1), dtype=np.uint32)
    rc = fm._L.debwt_fm_align_window(fm._h, buf, api._p64(offs), len(offs) - 1, ja, len(jobs), ctypes.byref(s),
                                     out.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmAln)),
                                     api._p64(coff) if with_offsets else None,
                                     cg.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), capacity)
    return rc, out, coff, cg


def test_capacity_protocol(api, plain):
    R, fm = plain
    pats, jobs = some_jobs(R, np.random.default_rng(12), count=10)
    full = fm.align_window(pats, jobs, scoring=SC_A)
    total = int(full.offsets[-1])
    assert total > 0
    rc, out, coff, _ = raw_call(api, fm, pats, jobs, SC_A, total - 1)
    assert rc == -5 and np.array_equal(coff, full.offsets) and out.tobytes() == full.aln.tobytes()
    assert "capacity" in fm._L.debwt_fm_last_error(fm._h).decode()
    rc, out, coff, cg = raw_call(api, fm, pats, jobs, SC_A, total)
    assert rc == 0 and np.array_equal(cg[:total], full.cigars)
    rc, *_ = raw_call(api, fm, pats, [], SC_A, 0)
    assert rc == 0


def test_invalid_arguments(api, plain):
    R, fm = plain
    rs = R.rs[1]
    pats = ["ACGTACGTAC", "", "A" * 4097, "C" * 4096]
    ok = (0, 0, 1, rs, rs + 100)
    assert len(fm.align_window(pats, [ok, (3, 1, 1, rs, rs + 16384)], cigar=False)) == 2     # the limits themselves
    bad = [(1, 0, 1, rs, rs + 100), (2, 0, 1, rs, rs + 100),                 # m = 0, m = 4097
           (0, 0, 1, rs + 100, rs + 99), (0, 0, 1, rs, rs + 16385),          # wend < wbeg, wider than 16384
           (4, 0, 1, rs, rs + 100), (0, 2, 1, rs, rs + 100), (0, 0, 4, rs, rs + 100)]   # pattern, strand, record
    for job in bad:
        for cigar in (True, False):
            with pytest.raises(api.DebwtError) as e:
                fm.align_window(pats, [ok, job], cigar=cigar)
            assert e.value.code == -1, job
    for sc in ((0, 4, 6, 1), (256, 4, 6, 1), (1, 0, 6, 1), (1, 256, 6, 1), (1, 4, -1, 1), (1, 4, 256, 1), (1, 4, 6, 0), (1, 4, 6, 256)):
        with pytest.raises(api.DebwtError) as e:
            fm.align_window(pats, [ok], scoring=sc)
        assert e.value.code == -1, sc


def test_no_text_attached(api):
    rng = np.random.default_rng(2)
    fm = index_of(api, [rng.integers(0, 4, size=200).astype(np.uint8)])
    with pytest.raises(api.DebwtError) as e:
        fm.align_window(["ACGTACGT"], [(0, 0, 0, 0, 100)])
    assert e.value.code == -4
    fm.close()
