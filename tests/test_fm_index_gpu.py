"""FM-index over built rows (debwt_fm_*, FMIndex): count and locate (in row order) against a numpy count of the text's
windows and a CPU suffix array, the full suffix array at s = 1 against that array, sum properties, indexes from saved
files, refusal of rows that are not the text's BWT, the per-pattern cap and batches cut inside the library."""
import numpy as np
import pytest

from conftest import golden_id, golden_manifest, golden_outputs, golden_records
from fm_definition import suffix_array

pytestmark = pytest.mark.gpu
MANIFEST = golden_manifest()
K32 = [e for e in MANIFEST if e["k"] == 32]
BIG = 2_000_000          # texts above this get fewer pattern lengths and fewer located patterns


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def text_of(recs):
    """symbols 0..3, 4 = '#', 5 = '$' of the records joined by separators; record start positions"""
    parts, starts, o = [], [], 0
    for r in recs:
        starts.append(o)
        parts.append(np.asarray(r, dtype=np.uint8))
        parts.append(np.array([4], dtype=np.uint8))
        o += len(r) + 1
    t = np.concatenate(parts)
    t[-1] = 5
    return t, np.array(starts, dtype=np.uint64)


class Windows:
    """every window of length L that holds no separator, sorted by its base-4 value; given the text's suffix array, the
    windows of one value stand in row order (by the suffix that begins there), as locate reports them"""

    def __init__(self, text, L, sa=None):
        n = len(text)
        m = n - L + 1
        v = np.zeros(m, dtype=np.uint64)
        bad = np.zeros(m, dtype=bool)
        sym = np.minimum(text, 3).astype(np.uint64)
        for j in range(L):
            v = v * np.uint64(4) + sym[j:j + m]
            bad |= text[j:j + m] > 3
        if sa is None:
            pos = np.nonzero(~bad)[0]
        else:
            pos = sa[sa < m]
            pos = pos[~bad[pos]]
        v, pos = v[pos], pos.astype(np.uint64)
        o = np.argsort(v, kind="stable")
        self.keys, self.pos, self.L = v[o], pos[o], L

    def lookup(self, codes):
        key = np.uint64(0)
        for c in codes:
            key = key * np.uint64(4) + np.uint64(c)
        a = np.searchsorted(self.keys, key, "left")
        b = np.searchsorted(self.keys, key, "right")
        return self.pos[a:b]


ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def ascii(codes, lower_mask=None):
    s = ACGT[np.asarray(codes, dtype=np.uint8)].copy()
    if lower_mask is not None:
        s[lower_mask] += 32
    return s.tobytes()


def sample_patterns(text, L, count, rng, mutate=0.1):
    """(ascii patterns, codes): windows of the text (some mutated, some in lower case) and random ones"""
    n = len(text)
    sep = np.nonzero(text > 3)[0]
    out = []
    tries = 0
    while len(out) < count and tries < 50 * count:
        tries += 1
        p = int(rng.integers(0, n - L))
        if np.searchsorted(sep, p) != np.searchsorted(sep, p + L):
            continue
        c = text[p:p + L].copy()
        if rng.random() < mutate:
            c[int(rng.integers(0, L))] = int(rng.integers(0, 4))
        out.append(c)
    for _ in range(max(count // 8, 2)):
        out.append(rng.integers(0, 4, size=L).astype(np.uint8))
    pats = [ascii(c, rng.random(L) < 0.2) for c in out]
    return pats, out


def check_index(fm, text, sa, rng, lengths, locate_every, cache):
    for L in lengths:
        if L not in cache:
            cache[L] = Windows(text, L, sa)
        W = cache[L]
        pats, codes = sample_patterns(text, L, 60, rng)
        cnt = fm.count(pats)
        want = [W.lookup(c) for c in codes]
        assert [int(x) for x in cnt] == [len(w) for w in want], L
        sel = list(range(0, len(pats), locate_every))
        got = fm.locate([pats[i] for i in sel])
        for g, i in zip(got, sel):
            assert np.array_equal(g, want[i]), (L, i)                  # in row order


@pytest.mark.parametrize("entry", K32, ids=golden_id)
def test_count_and_locate_against_windows(api, entry):
    recs = golden_records(entry)
    text, starts = text_of(recs)
    n = len(text)
    assert n == entry["n"]
    d = api.DeBWT(k=32)
    d.load_records(recs)
    d.build()
    rng = np.random.default_rng(n)
    big = n > BIG
    lengths = [1, 5, 12, 32] if big else [1, 2, 3, 5, 8, 13, 21, 32]
    sa = suffix_array(text)
    cache = {7: Windows(text, 7, sa)}
    for s in (1, 4, 32):
        fm = d.fm_index(sa_sample=s)
        info = fm.info()
        assert info["n"] == n and info["nrec"] == len(recs) and info["samples"] == (n + s - 1) // s
        assert np.array_equal(fm.record_starts(), starts)
        check_index(fm, text, sa, rng, lengths if s == 32 else lengths[-2:], 4 if big else 1, cache)
        # patterns that exist only across a separator, 'N' and empty patterns: 0
        cross = []
        for st in starts[1:6]:
            st = int(st)
            c = np.concatenate([text[st - 4:st - 1], text[st:st + 4]])
            if len(cache[7].lookup(c)) == 0:
                cross.append(ascii(c))
        odd = cross + [b"", b"N", b"ACGNT", b"acgtn", b"AC-GT"]
        assert not fm.count(odd).any()
        assert all(len(x) == 0 for x in fm.locate(odd))
        fm.close()
    # 100-base windows: the source is among the located positions, every position spells the pattern
    fm = d.fm_index(sa_sample=32)
    sep = np.nonzero(text > 3)[0]
    for _ in range(40):
        p = int(rng.integers(0, n - 100))
        if np.searchsorted(sep, p) != np.searchsorted(sep, p + 100):
            continue
        pat = ascii(text[p:p + 100])
        c = int(fm.count(pat)[0])
        loc = fm.locate(pat)[0]
        assert c == len(loc) and p in set(int(x) for x in loc)
        for q in loc:
            assert ascii(text[int(q):int(q) + 100]) == pat
        rec, off = fm.resolve(loc)
        assert np.array_equal(starts[rec] + off, loc)
    fm.close()
    d.close()


def test_full_suffix_array_at_s1(api):
    from debwt_amd import synth
    recs = synth.pan_genome(60_000, 6)
    text, _ = text_of(recs)
    n = len(text)
    d = api.DeBWT(k=32)
    d.load_records(recs)
    d.build()
    words, hrows, drow = d.fetch()
    fm = d.fm_index(sa_sample=1)
    sa = fm.samples().astype(np.int64)
    assert len(sa) == n and np.array_equal(np.sort(sa), np.arange(n))
    assert np.array_equal(sa, suffix_array(text))                  # the suffix array itself, every row
    L = ((words[np.arange(n) >> 5] >> (2 * (31 - (np.arange(n) & 31))).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)
    L[hrows.astype(np.int64)] = 4
    L[drow] = 5
    assert np.array_equal(L, text[(sa - 1) % n])
    # consecutive rows whose suffix starts with a base: non-decreasing over 64 symbols (cut after the first separator)
    idx = (sa[:, None] + np.arange(64)[None, :]) % n
    win = text[idx].astype(np.int8) + 1
    after = np.cumsum(win > 4, axis=1) - (win > 4)          # separators strictly before the column
    win[after > 0] = 0
    base = text[sa] < 4
    a, b = win[:-1][base[:-1] & base[1:]], win[1:][base[:-1] & base[1:]]
    diff = a != b
    first = np.argmax(diff, axis=1)
    has = diff.any(axis=1)
    rows = np.nonzero(has)[0]
    assert (a[rows, first[rows]] < b[rows, first[rows]]).all()
    fm.close()
    d.close()


def test_sum_properties_20mbp(api):
    from debwt_amd import synth
    recs = synth.pan_genome(5_000_000, 4)
    text, _ = text_of(recs)
    n = len(text)
    d = api.DeBWT(k=32)
    d.load_records(recs)
    d.build()
    census = d.bwt_census()
    fm = d.fm_index()
    kmers = [ascii([(i >> (2 * (5 - j))) & 3 for j in range(6)]) for i in range(4 ** 6)]
    windows6 = sum(len(r) - 5 for r in recs)
    assert int(fm.count(kmers).sum()) == windows6
    ones = fm.count([b"A", b"C", b"G", b"T"])
    want = census.copy()
    want[3] -= len(recs)
    assert np.array_equal(ones, want)
    assert np.array_equal(fm.info()["census"], census)
    # 'A' occurs > 4 M times: its locate is cut into several launches
    pos = fm.locate(b"a")[0]
    assert np.array_equal(np.sort(pos), np.nonzero(text == 0)[0].astype(np.uint64))
    fm.close()
    d.close()


def _golden_with_files():
    return [e for e in K32 if e.get("files")]


@pytest.mark.parametrize("entry", _golden_with_files()[:3], ids=golden_id)
def test_index_from_host_rows_and_from_files(api, entry):
    recs = golden_records(entry)
    text, starts = text_of(recs)
    words, hrows, drow = golden_outputs(entry)
    d = api.DeBWT(k=32)
    d.load_records(recs)
    d.build()
    own = d.fm_index(sa_sample=4)
    host = d.fm_index(sa_sample=4, rows=(words, hrows, drow))
    rng = np.random.default_rng(7)
    pats = sample_patterns(text, 9, 200, rng)[0] + sample_patterns(text, 3, 50, rng)[0]
    assert np.array_equal(own.ranges(pats), host.ranges(pats))
    samples = host.samples()
    assert np.array_equal(samples, own.samples())
    d.close()                                              # the indexes outlive the context
    opened = api.FMIndex.open(words, len(text), hrows, drow, samples, sa_sample=4)
    assert np.array_equal(opened.ranges(pats), own.ranges(pats))
    for a, b in zip(opened.locate(pats), own.locate(pats)):
        assert np.array_equal(a, b)
    sep = np.nonzero(text > 3)[0]
    assert np.array_equal(opened.record_starts(), np.concatenate([[0], sep[:-1] + 1]).astype(np.uint64))
    assert np.array_equal(opened.record_starts(), starts)
    for x in (own, host, opened):
        x.close()


def test_corrupted_rows_are_refused(api):
    from debwt_amd import synth
    recs = synth.pan_genome(40_000, 3)
    n = sum(len(r) for r in recs) + len(recs)
    d = api.DeBWT(k=32)
    d.load_records(recs)
    d.build()
    words, hrows, drow = d.fetch()
    rng = np.random.default_rng(11)
    bad = words.copy()
    while True:
        i, j = (int(x) for x in rng.integers(0, n, size=2))
        si = int(bad[i >> 5] >> np.uint64(2 * (31 - (i & 31)))) & 3
        sj = int(bad[j >> 5] >> np.uint64(2 * (31 - (j & 31)))) & 3
        if si != sj and i not in hrows and j not in hrows and drow not in (i, j):
            break
    for pos, s in ((i, sj), (j, si)):
        sh = np.uint64(2 * (31 - (pos & 31)))
        bad[pos >> 5] = (bad[pos >> 5] & ~(np.uint64(3) << sh)) | (np.uint64(s) << sh)
    with pytest.raises(api.DebwtError) as ei:
        d.fm_index(rows=(bad, hrows, drow))
    assert ei.value.code == -1 and "not the BWT" in str(ei.value)
    good = d.fm_index(rows=(words, hrows, drow))               # the context is unharmed
    assert int(good.count(b"ACGT")[0]) > 0
    good.close()
    with pytest.raises(api.DebwtError):
        d.fm_index(sa_sample=3)
    d.close()


def test_cap_and_large_batch(api):
    from debwt_amd import synth
    recs = synth.pan_genome(200_000, 3)
    text, _ = text_of(recs)
    d = api.DeBWT(k=32)
    d.load_records(recs)
    d.build()
    fm = d.fm_index(sa_sample=8)
    full = fm.locate([b"ACG", b"TTTT", b"GATTACA"])
    capped = fm.locate([b"ACG", b"TTTT", b"GATTACA"], max_per_pattern=5)
    for f, c in zip(full, capped):
        assert len(c) == min(5, len(f)) and np.array_equal(c, f[:len(c)])       # the first rows, in row order
    # 1.2 M patterns: more than one count launch
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 4, size=(1_200_000, 10)).astype(np.uint8)
    buf = ACGT[codes]
    pats = [bytes(r) for r in buf]
    cnt = fm.count(pats)
    W = Windows(text, 10)
    keys = np.zeros(len(codes), dtype=np.uint64)
    for j in range(10):
        keys = keys * np.uint64(4) + codes[:, j].astype(np.uint64)
    want = np.searchsorted(W.keys, keys, "right") - np.searchsorted(W.keys, keys, "left")
    assert np.array_equal(cnt, want.astype(np.uint64))
    fm.close()
    d.close()
