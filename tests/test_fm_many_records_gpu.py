"""Every FM query on an index of 2^24 + 300 + 3003 records (tests/many_records_ref.py): the rank lines behind the first
2^24 separator rows keep a non-zero high half of their separators-before count, and v_occ, fm_occ2 and fm_line_occ4 each
decode it on the way to the answers below; record numbers in da and in overlap hits pass 2^24, and one overlap query
returns more hits than one expansion launch writes.  The index is opened from the definition's rows, so the builder (which
takes no record of one base) is not in the way; tests/test_many_records_build_gpu.py covers the builder and the verifier at
this record count.  Every comparison is exact, against sa and sym of the definition; strings, mismatch counts, MEM spans
and overlap flags come from the brute force over the scaled instance with the same head.
tests/test_many_records_ref.py shows on the CPU that the patterns sent here need the high bits."""
import numpy as np
import pytest

import fm_definition as F
import many_records_ref as M
import spectrum_ref as SR
from test_fm_geometry_gpu import check_locate, check_ranges

pytestmark = pytest.mark.gpu
NA, NT = M.FULL
FIRST_A, FIRST_T = 3, 3 + NA                     # record numbers


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def opened(api, s):
    X = M.index()
    return api.FMIndex.open(X.words, X.n, X.hash_rows, X.dollar_row, F.samples(X.sa, s), sa_sample=s)


@pytest.fixture(scope="module")
def fm(api):
    x = opened(api, 32)
    yield x
    x.close()


@pytest.fixture(scope="module")
def ranges_want():
    X = M.index()
    return np.array([X.interval(p) for p in M.range_patterns()], dtype=np.uint64).reshape(-1, 2)


# ---- facts -------------------------------------------------------------------------------------------------------------

def test_index_facts(fm):
    X = M.index()
    info = fm.info()
    assert info["n"] == X.n and info["nrec"] == 3 + NA + NT == X.nrec and info["sa_sample"] == 32
    assert info["samples"] == (X.n + 31) // 32
    assert np.array_equal(info["census"], X.census())
    assert np.array_equal(fm.record_starts(), X.starts())
    assert np.array_equal(fm.samples(), F.samples(X.sa, 32))


# ---- ranges, count, locate ---------------------------------------------------------------------------------------------

def test_ranges_and_count(fm, ranges_want):
    X, pats = M.index(), M.range_patterns()
    check_ranges(fm.ranges(pats), ranges_want, pats)
    count = dict(zip(pats, (ranges_want[:, 1] - ranges_want[:, 0]).tolist()))
    assert np.array_equal(fm.count(pats), ranges_want[:, 1] - ranges_want[:, 0])
    inside = lambda w: sum(s[i:i + len(w)] == w for s in X.head_strs for i in range(len(s)))      # noqa: E731
    assert count[b"A"] == NA and count[b"T"] == NT + inside("T") and count[b"C"] == inside("C")
    assert count[b"AA"] == count[b"AT"] == count[b"TA"] == 0          # no pair spans a separator
    assert count[b"TT"] == inside("TT") > 0                            # the head's own: none from the one-base records
    assert count[b"N"] == count[b""] == count[b"CGNT"] == 0


def test_locate(fm, ranges_want):
    X, pats = M.index(), M.range_patterns()
    keep = [i for i, p in enumerate(pats) if p != b"A"]                  # 'A' whole in the next test
    some = [pats[i] for i in keep]
    check_locate(fm.locate(some), X.sa, ranges_want[keep], some)
    check_locate(fm.locate(pats, max_per_pattern=3), X.sa, ranges_want, pats, cap=3)


def test_locate_every_one_base_record(fm):
    X = M.index()
    got = fm.locate([b"A"])[0]
    assert len(got) == NA and np.array_equal(got.astype(np.int64), X.sa[:NA])
    rec, off = fm.resolve(got[[0, 1, M.HIGH - 4, M.HIGH - 3, M.HIGH - 2, NA - 1]])
    assert rec.tolist() == [3, 4, M.HIGH - 1, M.HIGH, M.HIGH + 1, 3 + NA - 1] and not off.any()


def locate_rows(api, fm, ranges):
    """debwt_fm_locate on row ranges that no pattern names"""
    r = np.ascontiguousarray(ranges, dtype=np.uint64).reshape(-1, 2)
    offs = np.zeros(len(r) + 1, dtype=np.uint64)
    pos = np.zeros(int((r[:, 1] - r[:, 0]).sum()), dtype=np.uint64)
    fm._chk(fm._L.debwt_fm_locate(fm._h, api._p64(r), len(r), 0, api._p64(offs), api._p64(pos), len(pos)))
    assert int(offs[-1]) == len(pos)
    return pos


def test_locate_walks_through_header_branch_lines(api):
    """sa_sample = 1024: a walk of up to 1023 LF steps.  From a head pattern's row it stays among the head's suffixes until
    a record's start; from a 'T' row of the last '#' suffixes it alternates between those rows and the T# rows."""
    X = M.index()
    x = opened(api, 1024)
    pats = M.locate_patterns()
    want = np.array([X.interval(p) for p in pats], dtype=np.uint64).reshape(-1, 2)
    assert (want[:, 1] > want[:, 0]).all()
    check_locate(x.locate(pats), X.sa, want, pats)
    rows = M.tail_t_rows(X)
    assert len(rows) == 64 and (rows % 1024 != 0).any()
    got = locate_rows(api, x, np.stack([rows, rows + 1], axis=1))
    assert np.array_equal(got.astype(np.int64), X.sa[rows])
    lines = X.high_lines(X.tail_rows)
    lo, hi = int(lines[0]) * M.ROWS, X.n                                  # every row of those lines, '$' included
    assert np.array_equal(locate_rows(api, x, [[lo, hi]]).astype(np.int64), X.sa[lo:hi])
    x.close()


# ---- search and MEMs ---------------------------------------------------------------------------------------------------

def test_search(fm):
    pats, ref = M.reads(), M.search_reference()
    assert sum(1 for r in ref for h in r if h[2] > 0) > 10 and sum(1 for r in ref for h in r if h[3] == 1) > 3
    for K in (0, 1, 2):
        for strands in ("forward", "both"):
            res = fm.search(pats, mismatches=K, strands=strands)
            assert len(res) == len(pats)
            for i, p in enumerate(pats):
                want = [h for h in ref[i] if h[2] <= K and (strands == "both" or h[3] == 0)]
                r, mm, st = res.hits(i)
                got = [(int(a), int(b), int(m), int(t)) for (a, b), m, t in zip(r.tolist(), mm.tolist(), st.tolist())]
                assert got == want, (K, strands, p)


def test_mems(fm):
    D, X = M.scaled(), M.index()
    reads = M.reads() + ("A", "T", "AT", "CATG")
    for min_len in (1, 19):
        for strands in ("forward", "both"):
            res = fm.mems(reads, min_len=min_len, strands=strands)
            assert len(res) == len(reads)
            total = 0
            for i, p in enumerate(reads):
                sp, rg, st = res.hits(i)
                got = [(int(t), int(a), int(b)) for (a, b), t in zip(sp.tolist(), st.tolist())]
                want = D.mems(p, min_len, strands == "both")
                assert got == want, (min_len, strands, p)
                for (t, a, b), r in zip(want, rg.tolist()):
                    w = p[a:b].upper()
                    assert tuple(r) == X.interval(w if t == 0 else F.revcomp(w)), (min_len, strands, p, t, a, b)
                total += len(want)
            assert total > 20


# ---- k-mers ------------------------------------------------------------------------------------------------------------

def test_kmer_counts(fm):
    X = M.index()
    reads = list(X.head_strs) + list(M.reads()) + ["", "A", "T", "a", "AT", "TA", "ACGTACGTACGTACGT", "T" * 14, "A" * 14]
    for k in (1, 2, 11, 12, 13):
        for strands in ("forward", "both"):
            R = M.kmer_ref(k, strands == "both")
            res = fm.kmer_counts(reads, k, strands=strands)
            assert len(res) == len(reads) and res.counts.dtype == np.uint32
            for i, p in enumerate(reads):
                assert res.profile(i).tolist() == R.profile(p), (k, strands, p[:40])
            assert fm.kmer_stats()["table_q"] == (12 if k >= 12 else 0)
    R = M.kmer_ref(1, True)
    assert R.cnt("A") == R.cnt("T") == NA + NT + sum(s.count("T") for s in X.head_strs)


def test_spectrum(fm):
    for k in (1, 2, 12):
        occ = M.kmer_occ(k)
        for strands in ("forward", "both"):
            D = SR.members_of(occ, strands == "both")
            res = fm.spectrum(k, strands=strands, bins=256)
            assert res.hist.tolist() == SR.histogram(D, 256), (k, strands)
            assert (res.distinct, res.total, res.overflow_total) == SR.totals(D, 256), (k, strands)


# ---- overlaps ----------------------------------------------------------------------------------------------------------

def overlaps_want(api, q, first, count):
    """The hits of the scaled instance, with its one-base records replaced by the `count` records from `first` on: they
    are the last hits (length 1, behind the head's records), all with one flags value"""
    D = M.scaled()
    small = D.overlaps(q, 1)
    head = [h for h in small if h[0] < 3]
    single = [h for h in small if h[0] >= 3]
    assert single and small == head + single and {h[1] for h in single} == {1} and len({h[3] for h in single}) == 1
    assert len(single) == (M.SCALED[0] if first == FIRST_A else M.SCALED[1])
    out = np.zeros(len(head) + count, dtype=api._OVERLAP_DTYPE)
    for j, h in enumerate(head):
        out[j] = h
    tail = out[len(head):]
    tail["record"], tail["length"], tail["flags"] = first + np.arange(count, dtype=np.uint32), 1, single[0][3]
    return out


def test_overlaps_more_hits_than_one_launch(api, fm):
    """a query that ends in 'A' lists every one-base 'A' record: more than 2^24 hits, record numbers up to 2^24 + 302"""
    X = M.index()
    q = X.head_strs[0][:20] + "A"
    want = overlaps_want(api, q, FIRST_A, NA)
    assert len(want) == NA and int(want["record"][-1]) == 3 + NA - 1 > M.HIGH
    res = fm.overlaps([q], min_overlap=1)
    st = fm.overlaps_stats()
    assert st["hits"] == NA and st["batches"] == 1
    assert st["launches"] == 2 + -(-NA // M.HIGH) == 4                    # the walk, the compaction, two expansion launches
    assert res.offsets.tolist() == [0, NA] and np.array_equal(res.all_hits, want)
    mm = fm.overlaps_mm([q], min_overlap=1, mismatches=0)
    assert np.array_equal(mm.offsets, res.offsets) and mm.all_hits.tobytes() == res.all_hits.tobytes()


def test_overlaps_t_records(api, fm):
    X = M.index()
    s = X.head_strs[1]
    k = s.index("T", 8) + 1
    queries = ["GG" + s[:k], "T", "t", "", X.head_strs[2][-12:] + "CT"]
    want = [overlaps_want(api, q, FIRST_T, NT) if q else np.zeros(0, dtype=api._OVERLAP_DTYPE) for q in queries]
    assert len(want[0]) > NT and int(want[0]["length"][0]) == k           # the head record the query was cut from
    assert int(want[1]["flags"][0]) == 3 and int(want[0]["flags"][-1]) == 1   # whole and contained; contained
    res = fm.overlaps(queries, min_overlap=1)
    assert res.offsets.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    for i, w in enumerate(want):
        assert np.array_equal(res.hits(i), w), queries[i]
    mm = fm.overlaps_mm(queries, min_overlap=1, mismatches=0)
    assert np.array_equal(mm.offsets, res.offsets) and mm.all_hits.tobytes() == res.all_hits.tobytes()


# ---- extract and restore -----------------------------------------------------------------------------------------------

def test_extract(fm):
    X = M.index()
    jobs, want = [], []

    def add(rec, off=None, length=None):
        s = X.record_string(rec)
        jobs.append((rec,) if off is None else (rec, off, length))
        want.append(s if off is None else s[off:off + length])

    starts = [0, len(X.head_strs[0]) + 1, len(X.head_strs[0]) + len(X.head_strs[1]) + 2]
    for r in range(3):
        add(r)
    for q in range(0, X.H - 1, 32):                                      # parts that begin or end on a multiple of 32
        r = max(j for j in range(3) if starts[j] <= q)
        off, m = q - starts[r], len(X.head_strs[r])
        add(r, 0, off)
        add(r, off, m - off)
        add(r, off, 32)
        if off >= 32:
            add(r, off - 32, 32)
    rng = np.random.default_rng(8)
    named = [3, 4, M.HIGH - 1, M.HIGH, M.HIGH + 1, FIRST_T - 1, FIRST_T, FIRST_T + 1, X.nrec - 1]
    for r in named + rng.integers(3, X.nrec, 1000 - len(named)).tolist():
        add(r)
    add(M.HIGH, 0, 1)
    add(M.HIGH, 1, 5)                                                   # behind the record's end: empty
    assert sum(1 for j in jobs if len(j) == 1 and j[0] >= FIRST_T) > 0
    got = fm.extract(jobs)
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w.encode(), (jobs[j], g[:40], w[:40])


def test_restore_text(api):
    X = M.index()
    x = opened(api, 32)
    x.restore_text()
    st = x.extract_stats()
    assert st["jobs"] == 0 and st["bases"] == X.n and st["steps"] == X.n - 1
    words, sep = F.packed_text_of(X.sym)
    w, sp = x.text()
    assert np.array_equal(w, words) and np.array_equal(sp, sep)
    x.close()


# ---- suffix array, record array, LCP array ------------------------------------------------------------------------------

def test_esa_and_record_counts(fm):
    X, E = M.index(), M.esa()
    e = fm.esa(sa=True, da=True)
    assert np.array_equal(e.sa().astype(np.int64), X.sa)
    da = e.da()
    assert da.dtype == np.uint32 and np.array_equal(da, E.da) and int(da.max()) == X.nrec - 1
    assert np.array_equal(e.lcp(), E.lcp())
    assert e.summary() == E.summary()
    assert e.profile(16).tolist() == E.profile(16)
    e.records_build()
    pats = [b"A", b"T"] + list(M.locate_patterns()[:60]) + list(M.range_patterns()[:40])
    rg = np.array([X.interval(p) for p in pats], dtype=np.uint64).reshape(-1, 2)
    want = [len(np.unique(E.da[int(lo):int(hi)])) for lo, hi in rg.tolist()]
    assert want[0] == NA and want[1] == NT + 3
    assert e.record_counts(rg).tolist() == want
    e.release()
