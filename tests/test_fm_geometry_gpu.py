"""The rank structure and every FM query on indexes opened from definition-built rows (tests/fm_definition.py): small
collections on the edges of the 384-row rank line -- n % 384 and n % 32 of 0 and 1, a line of separator rows only, lines
whose 'T' count comes from the header words, records of one base, an all-'T' text, the '$' row on row 0, 383 and 384 --
and the collections outside the builder's domain, at sa_sample 1, 2, 32 and 1024 (one sample, two above 1024 rows:
locate walks through the '$' row, extract has little more than the free anchors).  Every answer is compared with the
brute force over the record strings and the definition's suffix array; every comparison is exact.  The builder, the
verifier and the sample walk are run on the cases the builder accepts.  tests/test_fm_geometry_selfcheck.py runs these
assertions on the CPU against right and wrong answers.  The high 24 bits of a line's separators-before count are covered
by test_fm_many_records_gpu.py, on the index of many_records_ref.py."""
import functools

import numpy as np
import pytest

import fm_definition as F
from test_fm_search_gpu import brute_patterns

pytestmark = pytest.mark.gpu
CASES = list(F.geometry_cases())
SAMPLINGS = (1, 2, 32, 1024)
EINVAL = -1


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def opened(api, name, s):
    D = F.definition_of(name)
    fm = api.FMIndex.open(D.words, D.n, D.hash_rows, D.dollar_row, F.samples(D.sa, s), sa_sample=s)
    return D, fm


everywhere = pytest.mark.parametrize("s", SAMPLINGS)
every_case = pytest.mark.parametrize("name", CASES)


# ---- index facts -------------------------------------------------------------------------------------------------------

@everywhere
@every_case
def test_index_facts(api, name, s):
    D, fm = opened(api, name, s)
    info = fm.info()
    nsamp = (D.n + s - 1) // s
    assert info["n"] == D.n and info["nrec"] == D.nrec and info["sa_sample"] == s and info["samples"] == nsamp
    assert nsamp == (1 if D.n <= s else 2) or s < 1024          # at s = 1024: row 0 and, above 1024 rows, row 1024
    assert np.array_equal(info["census"], D.census())
    assert np.array_equal(fm.record_starts(), D.starts)
    assert np.array_equal(fm.samples(), D.sa[::s].astype(np.uint64))
    fm.close()


# ---- ranges and locate -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def range_reference(name):
    D = F.definition_of(name)
    return np.array([D.interval(p) for p in F.range_patterns(name)], dtype=np.uint64).reshape(-1, 2)


def check_ranges(got, want, pats):
    """row for row where the pattern occurs; hi == lo where it does not (the backward search stops early there, and lo is
    then no function of the pattern)"""
    assert got.shape == want.shape
    occurs = want[:, 1] > want[:, 0]
    bad = np.nonzero(occurs & (got != want).any(axis=1))[0]
    assert not len(bad), (pats[bad[0]], got[bad[0]].tolist(), want[bad[0]].tolist())
    bad = np.nonzero(~occurs & (got[:, 1] != got[:, 0]))[0]
    assert not len(bad), (pats[bad[0]], got[bad[0]].tolist())


def check_locate(got, sa, want, pats, cap=None):
    """the positions of every pattern's rows, in row order"""
    assert len(got) == len(want)
    for i, g in enumerate(got):
        lo, hi = int(want[i, 0]), int(want[i, 1])
        w = sa[lo:hi] if cap is None else sa[lo:hi][:cap]
        assert np.array_equal(g.astype(np.int64), w), (pats[i], g.tolist(), w.tolist())


@everywhere
@every_case
def test_ranges(api, name, s):
    D, fm = opened(api, name, s)
    pats, want = F.range_patterns(name), range_reference(name)
    check_ranges(fm.ranges(pats), want, pats)
    assert np.array_equal(fm.count(pats), want[:, 1] - want[:, 0])
    fm.close()


@everywhere
@every_case
def test_locate(api, name, s):
    D, fm = opened(api, name, s)
    pats, want = F.range_patterns(name), range_reference(name)
    check_locate(fm.locate(pats), D.sa, want, pats)
    check_locate(fm.locate(pats, max_per_pattern=3), D.sa, want, pats, cap=3)
    fm.close()


# ---- extract and restore -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def extract_jobs(name):
    """(jobs, expected strings): whole records, the first base, the last base and all of every record, 50 random
    substrings, and jobs that begin or end on a multiple of 32 in text coordinates (empty ones among them)"""
    D = F.definition_of(name)
    rng = np.random.default_rng(D.n + 1)
    jobs, want = [], []

    def add(rec, off=None, length=None):
        jobs.append((rec,) if off is None else (rec, off, length))
        want.append(D.substring(rec) if off is None else D.substring(rec, off, length))

    for r in range(D.nrec):
        m = len(D.strs[r])
        add(r)
        add(r, 0, 1)
        add(r, m - 1, 1)
        add(r, 0, m)
    for _ in range(50):
        r = int(rng.integers(0, D.nrec))
        m = len(D.strs[r])
        a = int(rng.integers(0, m))
        add(r, a, int(rng.integers(1, m - a + 1)))
    starts = D.starts.astype(np.int64)
    for q in range(0, D.n, 32):
        r = int(np.searchsorted(starts, q, side="right")) - 1
        off, m = q - int(starts[r]), len(D.strs[r])              # off == m: q is the record's separator
        add(r, 0, off)                                          # ends on q
        add(r, off, m - off)                                    # begins on q
        add(r, off, 32)                                         # to the next multiple, or clipped at the record's end
        if off >= 32:
            add(r, off - 32, 32)
    return tuple(jobs), tuple(w.encode() for w in want)


@everywhere
@every_case
def test_extract_and_restore(api, name, s):
    D, fm = opened(api, name, s)
    jobs, want = extract_jobs(name)
    got = fm.extract(jobs)
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, (jobs[j], g, w)
    words, sep = F.packed_text(D.records)
    fm.restore_text()
    st = fm.extract_stats()
    assert st["jobs"] == 0 and st["bases"] == D.n and st["steps"] == D.n - 1
    w, sp = fm.text()
    assert np.array_equal(w, words) and np.array_equal(sp, sep)
    assert fm.extract(jobs[:40]) == list(want[:40])              # anchors and text side by side
    fm.close()


# ---- k-mer counts ------------------------------------------------------------------------------------------------------

@every_case
def test_kmer_counts(api, name):
    D, fm = opened(api, name, 32)
    longest = max(D.strs, key=len)
    reads = list(D.strs) + ["", longest[:1], longest[:10], longest[:11], longest[:12], longest[:13], longest.lower(),
                            longest[:5] + "N" + longest[6:], "ACGTACGTACGTACGT", "T" * 14]
    for k in (1, 2, 11, 12, 13):
        for strands in ("forward", "both"):
            res = fm.kmer_counts(reads, k, strands=strands)
            assert len(res) == len(reads)
            assert res.counts.dtype == np.uint32                # clamped at 2^32 - 1: the reference clamps as well
            for i, p in enumerate(reads):
                want = D.kmer_profile(p, k, strands == "both")
                assert res.profile(i).tolist() == want, (k, strands, p)
            st = fm.kmer_stats()
            assert st["table_q"] == (12 if k >= 12 else 0)
    fm.close()


# ---- overlaps ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def overlap_queries(name):
    """the records, and suffixes of up to 50 of them cut around the min_overlap values and at both ends"""
    D = F.definition_of(name)
    q = list(D.strs)
    step = max(1, D.nrec // 50)
    for s in D.strs[::step][:50]:
        m = len(s)
        for a in sorted({1, m // 2, m - 41, m - 40, m - 39, m - 9, m - 8, m - 7, m - 2, m - 1}):
            if 0 < a < m:
                q.append(s[a:])
    q += [D.strs[0].lower(), "N" + D.strs[0], D.strs[0] + "N", ""]
    return tuple(dict.fromkeys(q))                               # equal queries have equal answers: each once


@functools.lru_cache(maxsize=None)
def overlap_reference(name, min_overlap):
    """per query the exact overlaps on both strands; the forward ones are those of strand 0"""
    D = F.definition_of(name)
    return tuple(tuple(D.overlaps(q, min_overlap, both=True)) for q in overlap_queries(name))


@functools.lru_cache(maxsize=None)
def overlap_mm_reference(name):
    """per query (of at most 1024 bytes) and strand the hits at K = 2 and min_overlap = 1: a smaller K or a larger
    min_overlap keeps the hits within it, in the same order"""
    D = F.definition_of(name)
    return tuple((F.overlap_mm_brute(D.strs, q, 1, 2, 0, 0), F.overlap_mm_brute(D.strs, F.revcomp(q), 1, 2, 0, 1))
                 for q in overlap_queries(name) if len(q) <= 1024)


def tuples(res, i):
    return [tuple(int(x) for x in h) for h in res.hits(i).tolist()]


@everywhere
@every_case
def test_overlaps(api, name, s):
    D, fm = opened(api, name, s)
    queries = overlap_queries(name)
    short = [q for q in queries if len(q) <= 1024]
    if len(short) < len(queries):                                # overlaps_mm takes patterns of at most 1024 bytes
        with pytest.raises(api.DebwtError) as e:
            fm.overlaps_mm(queries, min_overlap=8, mismatches=1)
        assert e.value.code == EINVAL
    mm_ref = overlap_mm_reference(name)
    for min_overlap in (1, 8, 40):
        slots = sum(max(0, len(q) - min_overlap + 1) for q in queries)
        for strands in ("forward", "both"):
            both = strands == "both"
            for longest in (False, True):
                res = fm.overlaps(queries, min_overlap=min_overlap, strands=strands, longest=longest)
                assert len(res) == len(queries)
                ref = overlap_reference(name, min_overlap)
                for i, q in enumerate(queries):
                    want = [h for h in ref[i] if both or h[2] == 0]
                    assert tuples(res, i) == (F.longest_of(want) if longest else want), (min_overlap, strands, longest, q)
                if not slots:                                    # every query is shorter than min_overlap
                    assert len(res.all_hits) == 0 and fm.overlaps_stats()["runs"] == 0
                exact = fm.overlaps(short, min_overlap=min_overlap, strands=strands, longest=longest)
                for K in (0, 1, 2):
                    got = fm.overlaps_mm(short, min_overlap=min_overlap, mismatches=K, strands=strands, longest=longest)
                    if K == 0:
                        assert np.array_equal(got.offsets, exact.offsets) and np.array_equal(got.all_hits, exact.all_hits)
                    for i, q in enumerate(short):
                        want = [h for h in mm_ref[i][0] + (mm_ref[i][1] if both else [])
                                if h[1] >= min_overlap and h[3] >> 8 <= K]
                        if longest:
                            want = F.longest_of(want)
                        assert tuples(got, i) == want, (min_overlap, K, strands, longest, q)
    fm.close()


# ---- search and MEMs ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def search_reference(name):
    """(patterns, per pattern the hits at K = 2 on both strands): 60 patterns taken as test_fm_search_gpu.brute_patterns
    takes them; a hit is one distinct text string, so a smaller K keeps the hits within it"""
    D = F.definition_of(name)
    rng = np.random.default_rng(D.n + 2)
    pats = brute_patterns(D.sym, rng, 3)
    if len(pats) > 60:
        pats = [pats[int(i)] for i in np.sort(rng.choice(len(pats), 60, replace=False))]
    return tuple(pats), tuple(D.search(p.decode(), 2, both=True) for p in pats)


@everywhere
@every_case
def test_search(api, name, s):
    D, fm = opened(api, name, s)
    pats, ref = search_reference(name)
    for K in (0, 1, 2):
        for strands in ("forward", "both"):
            for best in (False, True):
                res = fm.search(pats, mismatches=K, strands=strands, best=best)
                assert len(res) == len(pats)
                for i, p in enumerate(pats):
                    want = [h for h in ref[i] if h[2] <= K and (strands == "both" or h[3] == 0)]
                    if best and want:
                        least = min(h[2] for h in want)
                        want = [h for h in want if h[2] == least]
                    r, mm, st = res.hits(i)
                    got = [(int(a), int(b), int(m), int(t)) for (a, b), m, t in zip(r.tolist(), mm.tolist(), st.tolist())]
                    assert got == want, (K, strands, best, p)
    fm.close()


@functools.lru_cache(maxsize=None)
def mem_reads(name):
    """the records and mutated copies: substitutions, an N in every third, every fourth in lower case"""
    D = F.definition_of(name)
    rng = np.random.default_rng(D.n + 3)
    reads = list(D.strs)
    for i, s in enumerate(D.strs):
        t = list(s)
        for _ in range(1 + len(t) // 50):
            j = int(rng.integers(0, len(t)))
            t[j] = F.ACGT[(F.ACGT.index(t[j]) + 1 + int(rng.integers(0, 3))) % 4] if t[j] in F.ACGT else t[j]
        if i % 3 == 0 and len(t) >= 10:
            t[int(rng.integers(0, len(t)))] = "N"
        m = "".join(t)
        reads.append(m.lower() if i % 4 == 0 else m)
    return tuple(reads)


@everywhere
@every_case
def test_mems(api, name, s):
    D, fm = opened(api, name, s)
    reads = mem_reads(name)
    for min_len in (1, 5, 19):
        for strands in ("forward", "both"):
            res = fm.mems(reads, min_len=min_len, strands=strands)
            assert len(res) == len(reads)
            for i, p in enumerate(reads):
                sp, rg, st = res.hits(i)
                got = [(int(t), int(a), int(b)) for (a, b), t in zip(sp.tolist(), st.tolist())]
                want = D.mems(p, min_len, strands == "both")
                assert got == want, (min_len, strands, p)
                for (t, a, b), r in zip(want, rg.tolist()):
                    w = p[a:b].upper()
                    assert tuple(r) == D.interval(w if t == 0 else F.revcomp(w)), (min_len, strands, p, t, a, b)
    fm.close()


# ---- the builder, the verifier and the sample walk on the cases the builder takes ---------------------------------------

@pytest.mark.parametrize("name", F.BUILDER_CASES)
def test_builder_cross_check(api, name):
    D = F.definition_of(name)
    assert min(len(r) for r in D.records) > 32
    d = api.DeBWT(k=32)
    d.load_records(D.records)
    d.build()
    words, hrows, drow = d.fetch()
    assert np.array_equal(words, D.words) and np.array_equal(hrows, D.hash_rows) and drow == D.dollar_row
    assert d.verify_device()["inverse_bwt_ok"]
    assert np.array_equal(d.bwt_census(), D.census())
    for s in (1, 32):
        fm = d.fm_index(sa_sample=s)
        assert np.array_equal(fm.samples(), D.sa[::s].astype(np.uint64)), s
        pats, want = F.range_patterns(name), range_reference(name)
        check_ranges(fm.ranges(pats), want, pats)
        fm.close()
    d.close()
