"""FM-index search with up to K mismatches (debwt_fm_search, FMIndex.search): K = 0 against count, every hit located
and compared with a numpy Hamming scan of the text on both strands, best-only strata, tiny scratch buffers, errors,
indexes from files and 20 Mbp with batches cut inside the library."""
import ctypes

import numpy as np
import pytest

from conftest import golden_id, golden_manifest, golden_outputs, golden_records
from test_fm_index_gpu import ascii, sample_patterns, text_of

pytestmark = pytest.mark.gpu
MANIFEST = golden_manifest()
K32 = [e for e in MANIFEST if e["k"] == 32]
BRUTE = ["homopolymers_tandem", "special_branches", "shared_ends_duplicates", "lowercase_3x2500", "pan_4x20k",
         "reads_20000"]
COMP = np.array([3, 2, 1, 0] + [9] * 6, dtype=np.uint8)     # codes: A<->T, C<->G; 9 = a character that matches nothing


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def entry_named(name):
    return [e for e in K32 if e["name"] == name][0]


def index_of(api, recs, s=8):
    d = api.DeBWT(k=32)
    d.load_records(recs)
    d.build()
    fm = d.fm_index(sa_sample=s)
    d.close()
    return fm


def codes_of(p):
    """pattern bytes -> codes 0..3, 9 for anything outside ACGTacgt"""
    b = np.frombuffer(p, dtype=np.uint8) | 0x20 if len(p) else np.zeros(0, np.uint8)
    c = np.full(len(b), 9, dtype=np.uint8)
    for i, ch in enumerate(b"acgt"):
        c[b == ch] = i
    return c


class Text:
    def __init__(self, text):
        self.t = text
        sep = (text > 3).astype(np.int64)
        self.csep = np.concatenate([[0], np.cumsum(sep)])

    def scan(self, codes, K):
        """{position: distance} of every separator-free window with Hamming distance <= K"""
        m, n = len(codes), len(self.t)
        if m == 0 or m > n:
            return {}
        w = n - m + 1
        dist = np.zeros(w, dtype=np.uint8)
        for j in range(m):
            dist += self.t[j:j + w] != codes[j]
        ok = (self.csep[m:m + w] - self.csep[:w] == 0) & (dist <= K)
        p = np.nonzero(ok)[0]
        return dict(zip(p.tolist(), dist[p].tolist()))

    def expected(self, codes, K, both):
        """sorted (position, strand, mismatches) of both strands' windows"""
        out = [(p, 0, d) for p, d in self.scan(codes, K).items()]
        if both:
            out += [(p, 1, d) for p, d in self.scan(COMP[codes[::-1]], K).items()]
        return sorted(out)


def located(fm, res):
    return [sorted(zip(p.tolist(), s.tolist(), m.tolist())) for p, s, m in res.locate()]


def check_structure(res, K):
    """hits ordered by (strand, mismatches, lo), intervals non-empty and disjoint per (pattern, strand)"""
    for i in range(len(res)):
        r, mm, st = res.hits(i)
        assert np.all(r[:, 1] > r[:, 0]) and np.all(mm <= K)
        key = list(zip(st.tolist(), mm.tolist(), r[:, 0].tolist()))
        assert key == sorted(key)
        for s in (0, 1):
            iv = sorted(map(tuple, r[st == s].tolist()))
            assert all(a[1] <= b[0] for a, b in zip(iv, iv[1:]))


def brute_patterns(text, rng, count, lengths=(1, 2, 3, 5, 8, 13, 21, 40, 64)):
    """windows (mutated, lowercase), random patterns and patterns with N, as bytes"""
    pats = []
    for L in lengths:
        if L >= len(text):
            continue
        ps, codes = sample_patterns(text, L, count, rng, mutate=0.5)
        pats += ps
        for c in codes[:2]:
            c = c.copy()
            c[int(rng.integers(0, L))] = (int(c[0]) + 1) % 4
            pats.append(ascii(c))
        s = bytearray(ps[0])
        s[int(rng.integers(0, L))] = ord("N")
        pats.append(bytes(s))
    return pats


@pytest.mark.parametrize("entry", K32, ids=golden_id)
def test_k0_equals_count(api, entry):
    recs = golden_records(entry)
    text, _ = text_of(recs)
    fm = index_of(api, recs, s=32)
    rng = np.random.default_rng(len(text))
    pats = []
    for L in (1, 4, 11, 32):
        pats += sample_patterns(text, L, 40, rng)[0]
    pats += [b"", b"ACGTN", b"acgtacgt", b"N", b"AXA"]
    res = fm.search(pats, mismatches=0)
    want = fm.ranges(pats)
    for i in range(len(pats)):
        r, mm, st = res.hits(i)
        if want[i, 1] > want[i, 0]:
            assert len(r) == 1 and tuple(r[0]) == tuple(want[i]) and mm[0] == 0 and st[0] == 0, pats[i]
        else:
            assert len(r) == 0, pats[i]
    assert np.array_equal(res.count(), fm.count(pats))
    fm.close()


@pytest.mark.parametrize("name", BRUTE)
def test_brute_force(api, name):
    entry = entry_named(name)
    recs = golden_records(entry)
    text, _ = text_of(recs)
    T = Text(text)
    big = len(text) > 1_000_000
    fm = index_of(api, recs, s=1 if len(text) < 10_000 else 8)
    rng = np.random.default_rng(11)
    pats = brute_patterns(text, rng, 1 if big else 3, (13, 21, 40) if big else (1, 2, 3, 5, 8, 13, 21, 40, 64))
    pats += [b"N" * 3, b"ACNNT"]
    codes = [codes_of(p) for p in pats]
    for K in (1, 2, 3):
        for both in (False, True):
            if big and K == 3:
                continue
            res = fm.search(pats, mismatches=K, strands="both" if both else "forward")
            check_structure(res, K)
            got = located(fm, res)
            cnt = res.count()
            for i, c in enumerate(codes):
                if len(c) <= 2 and K >= len(c):       # every window of the text: compared through the count
                    assert int(cnt[i]) == len(T.expected(c, K, both)), (name, K, both, pats[i])
                    continue
                want = T.expected(c, K, both)
                assert got[i] == want, (name, K, both, pats[i])
                assert int(cnt[i]) == len(want)
    fm.close()


@pytest.mark.parametrize("name", ["homopolymers_tandem", "shared_ends_duplicates", "pan_4x20k"])
def test_best_only(api, name):
    recs = golden_records(entry_named(name))
    text, _ = text_of(recs)
    T = Text(text)
    fm = index_of(api, recs)
    rng = np.random.default_rng(5)
    pats = brute_patterns(text, rng, 3, (5, 8, 13, 21, 40))
    for K in (1, 2, 3):
        res = fm.search(pats, mismatches=K, strands="both", best=True)
        got = located(fm, res)
        for i, p in enumerate(pats):
            want = T.expected(codes_of(p), K, True)
            if want:
                low = min(w[2] for w in want)
                want = [w for w in want if w[2] == low]
            assert got[i] == want, (name, K, p)
            if fm.count([p])[0] > 0:
                assert set(res.hits(i)[1].tolist()) == {0}
    fm.close()


def test_bounded_scratch(api, monkeypatch):
    from debwt_amd import synth
    cases = []
    recs = golden_records(entry_named("homopolymers_tandem"))
    cases.append((recs, 3, brute_patterns(text_of(recs)[0], np.random.default_rng(3), 3, (8, 13, 21, 40))))
    g = synth.base_genome(200_000, seed=9, lowcx_fraction=0.3)
    recs2 = [g]
    t2 = text_of(recs2)[0]
    cases.append((recs2, 2, brute_patterns(t2, np.random.default_rng(4), 20, (12, 20, 30))))
    for recs, K, pats in cases:
        fm = index_of(api, recs)
        monkeypatch.delenv("DEBWT_FM_SEARCH_ITEMS", raising=False)
        ref = fm.search(pats, mismatches=K, strands="both")
        monkeypatch.setenv("DEBWT_FM_SEARCH_ITEMS", "300")
        small = fm.search(pats, mismatches=K, strands="both")
        st = fm.search_stats()
        assert st["retries"] > 0 and st["scratch_bytes"] <= (K + 1) * (4 * 1024 + 64) * 24
        monkeypatch.delenv("DEBWT_FM_SEARCH_ITEMS")
        for a in ("offsets", "ranges", "mismatches", "strands"):
            assert np.array_equal(getattr(ref, a), getattr(small, a)), a
        assert int(ref.offsets[-1]) > len(pats)
        fm.close()


def test_errors(api):
    from debwt_amd import _lib
    recs = golden_records(entry_named("shared_ends_duplicates"))
    fm = index_of(api, recs)
    with pytest.raises(api.DebwtError) as e:
        fm.search(["ACGT"], mismatches=5)
    assert e.value.code == -1
    with pytest.raises(api.DebwtError) as e:
        fm.search(["A" * 1025], mismatches=1)
    assert e.value.code == -1 and "1024" in str(e.value)
    fm.search(["A" * 1024], mismatches=1)
    text, _ = text_of(recs)
    pats = sample_patterns(text, 12, 40, np.random.default_rng(2))[0]
    buf = b"".join(pats)
    offs = np.zeros(len(pats) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in pats], out=offs[1:])
    L = _lib.lib()
    hoff = np.zeros(len(pats) + 1, dtype=np.uint64)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    one = np.zeros((1, 2), dtype=np.uint64)
    info1 = np.zeros(1, dtype=np.uint32)
    rc = L.debwt_fm_search(fm._h, buf, api._p64(offs), len(pats), 2, 1, api._p64(hoff), api._p64(one),
                           info1.ctypes.data_as(u32p), 1)
    total = int(hoff[-1])
    assert rc == -5 and total > 1
    ranges = np.zeros((total, 2), dtype=np.uint64)
    info = np.zeros(total, dtype=np.uint32)
    hoff2 = np.zeros_like(hoff)
    rc = L.debwt_fm_search(fm._h, buf, api._p64(offs), len(pats), 2, 1, api._p64(hoff2), api._p64(ranges),
                           info.ctypes.data_as(u32p), total)
    assert rc == 0 and np.array_equal(hoff, hoff2)
    res = fm.search(pats, mismatches=2, strands="both")
    assert np.array_equal(res.offsets, hoff) and np.array_equal(res.ranges, ranges)
    assert np.array_equal(res.mismatches, info & 0xFF) and np.array_equal(res.strands, info >> 8)
    fm.close()


def test_index_from_files(api):
    entry = entry_named("lowercase_3x2500")
    recs = golden_records(entry)
    text, _ = text_of(recs)
    words, hrows, drow = golden_outputs(entry)
    own = index_of(api, recs, s=4)
    opened = api.FMIndex.open(words, len(text), hrows, drow, own.samples(), sa_sample=4)
    pats = brute_patterns(text, np.random.default_rng(8), 4, (6, 15, 30))
    for best in (False, True):
        a = own.search(pats, mismatches=2, strands="both", best=best)
        b = opened.search(pats, mismatches=2, strands="both", best=best)
        for k in ("offsets", "ranges", "mismatches", "strands"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert located(own, a) == located(opened, b)
    own.close(); opened.close()


def test_scale_20mbp(api, monkeypatch):
    from debwt_amd import synth
    recs = synth.pan_genome(5_000_000, 4)
    text, _ = text_of(recs)
    T = Text(text)
    fm = index_of(api, recs, s=16)
    rng = np.random.default_rng(20)
    pats = []
    while len(pats) < 10_000:
        L = int(rng.integers(16, 25))
        ps, _ = sample_patterns(text, L, 64, rng, mutate=0.5)
        pats += ps
    pats = pats[:10_000]
    monkeypatch.setenv("DEBWT_FM_SEARCH_BATCH", "3000")
    monkeypatch.setenv("DEBWT_FM_SEARCH_ITEMS", "20000")
    res = fm.search(pats, mismatches=2, strands="both")
    st = fm.search_stats()
    assert st["batches"] == 4 and st["patterns"] == 10_000
    monkeypatch.delenv("DEBWT_FM_SEARCH_BATCH")
    monkeypatch.delenv("DEBWT_FM_SEARCH_ITEMS")
    check_structure(res, 2)
    assert np.array_equal(res.offsets, fm.search(pats, mismatches=2, strands="both").offsets)
    loc = res.locate(max_per_pattern=50)
    for i, (p, s, m) in enumerate(loc):                      # soundness: every located window has its distance
        c = codes_of(pats[i])
        for pos, strand, mm in zip(p.tolist(), s.tolist(), m.tolist()):
            q = c if strand == 0 else COMP[c[::-1]]
            w = text[pos:pos + len(q)]
            assert len(w) == len(q) and np.all(w <= 3) and int(np.sum(w != q)) == mm, (i, pos)
    for i in rng.choice(len(pats), 50, replace=False):        # completeness
        p = pats[int(i)]
        sub = fm.search([p], mismatches=2, strands="both")
        want = T.expected(codes_of(p), 2, True)
        assert located(fm, sub)[0] == want
        a, b = int(res.offsets[i]), int(res.offsets[i + 1])
        assert np.array_equal(res.ranges[a:b], sub.ranges)
    fm.close()
