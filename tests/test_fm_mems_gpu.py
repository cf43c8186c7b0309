"""Maximal exact matches (debwt_fm_mems, FMIndex.mems): spans against a Python reference computed from the definition
(s(e) by substring tests on the records), every MEM's interval against FMIndex.ranges and its located positions against
the brute-force occurrences, min_len filtering, strand symmetry, batches cut by tiny slot limits, errors and the
capacity protocol, indexes from files, and 20 Mbp checked through count."""
import ctypes

import numpy as np
import pytest

from conftest import golden_outputs, golden_records
from test_fm_index_gpu import text_of
from test_fm_search_gpu import BRUTE, entry_named, index_of

pytestmark = pytest.mark.gpu
COMP = str.maketrans("ACGTacgt", "TGCAtgca")


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def revcomp(p):
    return "".join(c.translate(COMP) if c in "ACGTacgt" else "N" for c in reversed(p))


def rec_strings(recs):
    return ["".join("ACGT"[c] for c in np.asarray(r).tolist()) for r in recs]


class Ref:
    """MEMs straight from the definition over the records joined by '#' (a string of A/C/G/T never spans a '#')"""

    def __init__(self, recs):
        self.strs = rec_strings(recs)
        self.text = "#".join(self.strs) + "$"

    def occurs(self, w):
        return w in self.text

    def s_of(self, q):
        """s(e) for every e of q (upper case), by a two-pointer walk: s is non-decreasing in e"""
        s, out = 0, []
        for e in range(len(q)):
            s = max(s, 0)
            while s <= e and not self.occurs(q[s:e + 1]):
                s += 1
            out.append(s)
        return out

    def mems(self, p, min_len, both):
        """sorted (strand, qbeg, qend) in the coordinates of p"""
        out = []
        m = len(p)
        for strand, q in ((0, p.upper()), (1, revcomp(p).upper())):
            if strand and not both:
                break
            s = self.s_of(q)
            for e in range(m):
                if s[e] <= e and (e == m - 1 or s[e + 1] > s[e]) and e + 1 - s[e] >= min_len:
                    a, b = s[e], e + 1
                    out.append((strand, a, b) if strand == 0 else (strand, m - b, m - a))
        return sorted(out)

    def positions(self, w):
        """global text positions of w (records joined by one separator each, as text_of lays them out)"""
        out, i = [], self.text.find(w)
        while i >= 0:
            out.append(i)
            i = self.text.find(w, i + 1)
        return out


def triples(res, i):
    sp, _, st = res.hits(i)
    return [(int(s), int(a), int(b)) for (a, b), s in zip(sp.tolist(), st.tolist())]


def mem_string(p, strand, a, b):
    w = p[a:b].upper()
    return w if strand == 0 else revcomp(w).upper()


def brute_patterns(strs, rng):
    """substrings with substitutions, insertions, deletions and N's, chimeras of two records, reads off a record's end,
    random strings, all-N, empty and one pattern longer than every record"""
    pats = []
    recs = [r for r in strs if len(r) >= 8]
    for _ in range(24):
        r = recs[int(rng.integers(0, len(recs)))]
        L = int(rng.integers(8, min(len(r), 120) + 1))
        a = int(rng.integers(0, len(r) - L + 1))
        s = list(r[a:a + L])
        for _ in range(int(rng.integers(0, 4))):
            kind, j = int(rng.integers(0, 4)), int(rng.integers(0, len(s)))
            if kind == 0:
                s[j] = "ACGT"[int(rng.integers(0, 4))]
            elif kind == 1:
                s.insert(j, "ACGT"[int(rng.integers(0, 4))])
            elif kind == 2 and len(s) > 2:
                del s[j]
            else:
                s[j] = "N"
        p = "".join(s)
        pats.append(p.lower() if rng.random() < 0.2 else p)
    for _ in range(6):                                        # chimeras of two records
        r1, r2 = (recs[int(rng.integers(0, len(recs)))] for _ in range(2))
        a, b = int(rng.integers(0, len(r1) - 4)), int(rng.integers(0, len(r2) - 4))
        pats.append(r1[a:a + 30] + r2[b:b + 30])
    for _ in range(4):                                        # off a record's end
        r = recs[int(rng.integers(0, len(recs)))]
        tail = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, 12))
        pats.append(r[-20:] + tail)
    for L in (1, 5, 17, 40):
        pats.append("".join("ACGT"[int(x)] for x in rng.integers(0, 4, L)))
    pats += ["N" * 9, "", "ACGTNNacgt"]
    longest = max(len(r) for r in strs)
    pats.append(strs[0][: min(len(strs[0]), 300)] + "ACGT" * ((longest + 3) // 4 + 1))
    return pats


@pytest.mark.parametrize("name", BRUTE)
def test_brute_force(api, name):
    recs = golden_records(entry_named(name))
    text, _ = text_of(recs)
    R = Ref(recs)
    fm = index_of(api, recs, s=1 if len(text) < 10_000 else 8)
    pats = brute_patterns(R.strs, np.random.default_rng(17))
    res = fm.mems(pats, min_len=1, strands="both")
    assert len(res) == len(pats)
    strings, per = [], []
    for i, p in enumerate(pats):
        got = triples(res, i)
        assert got == R.mems(p, 1, True), (name, p)
        assert got == sorted(got)
        for s, a, b in got:
            strings.append(mem_string(p, s, a, b))
    if not strings:
        return
    assert np.array_equal(res.ranges, fm.ranges(strings))
    cnt = res.count()
    few = [j for j in range(len(strings)) if cnt[j] <= 400]
    loc = res.locate()
    for j in few:
        assert sorted(loc[j].tolist()) == R.positions(strings[j]), (name, strings[j])
    capped = res.locate(max_per_mem=3)
    assert all(len(c) == min(int(n), 3) for c, n in zip(capped, cnt))
    fm.close()


@pytest.mark.parametrize("name", ["homopolymers_tandem", "shared_ends_duplicates", "pan_4x20k"])
def test_min_len_filters(api, name):
    recs = golden_records(entry_named(name))
    fm = index_of(api, recs)
    pats = brute_patterns(rec_strings(recs), np.random.default_rng(23))
    full = fm.mems(pats, min_len=1, strands="both")
    for L in (2, 12, 19, 40):
        r = fm.mems(pats, min_len=L, strands="both")
        for i in range(len(pats)):
            sp, rg, st = full.hits(i)
            keep = (sp[:, 1] - sp[:, 0]) >= L
            sp2, rg2, st2 = r.hits(i)
            assert np.array_equal(sp[keep], sp2) and np.array_equal(rg[keep], rg2) and np.array_equal(st[keep], st2)
    assert fm.mems(pats).offsets.tolist() == fm.mems(pats, min_len=19, strands="forward").offsets.tolist()
    fm.close()


def test_strand_symmetry(api):
    recs = golden_records(entry_named("pan_4x20k"))
    fm = index_of(api, recs)
    pats = brute_patterns(rec_strings(recs), np.random.default_rng(29))
    both = fm.mems(pats, min_len=1, strands="both")
    rc = fm.mems([revcomp(p) for p in pats], min_len=1, strands="forward")
    for i, p in enumerate(pats):
        m = len(p)
        sp, rg, st = both.hits(i)
        sp_r, rg_r, _ = rc.hits(i)
        one = st == 1
        mirrored = sorted((m - int(b), m - int(a)) for a, b in sp_r.tolist())
        assert [tuple(x) for x in sp[one].tolist()] == mirrored, p
        assert sorted(map(tuple, rg[one].tolist())) == sorted(map(tuple, rg_r.tolist()))
    fm.close()


def test_batches_do_not_change_results(api, monkeypatch):
    recs = golden_records(entry_named("pan_4x20k"))
    strs = rec_strings(recs)
    fm = index_of(api, recs)
    pats = brute_patterns(strs, np.random.default_rng(31)) + [strs[1][:900]]
    monkeypatch.delenv("DEBWT_FM_MEM_SLOTS", raising=False)
    ref = fm.mems(pats, min_len=1, strands="both")
    assert fm.mems_stats()["batches"] == 1
    for slots in ("1", "50", "700"):
        monkeypatch.setenv("DEBWT_FM_MEM_SLOTS", slots)
        small = fm.mems(pats, min_len=1, strands="both")
        st = fm.mems_stats()
        assert st["batches"] > 3 and st["mems"] == len(ref.spans)
        for a in ("offsets", "spans", "ranges", "strands"):
            assert np.array_equal(getattr(ref, a), getattr(small, a)), (slots, a)
    monkeypatch.setenv("DEBWT_FM_MEM_SLOTS", "50")            # the 900-base pattern needs 1800 slots: alone in its batch
    one = fm.mems([strs[1][:900]], min_len=1, strands="both")
    assert triples(one, 0)[0] == (0, 0, 900)
    fm.close()


def test_errors_and_capacity(api):
    from debwt_amd import _lib
    recs = golden_records(entry_named("shared_ends_duplicates"))
    fm = index_of(api, recs)
    pats = [p.encode() for p in brute_patterns(rec_strings(recs), np.random.default_rng(37)) if p]
    buf = b"".join(pats)
    offs = np.zeros(len(pats) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in pats], out=offs[1:])
    L = _lib.lib()
    n = len(pats)
    moff = np.zeros(n + 1, dtype=np.uint64)
    u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)

    def call(o, min_len, flags, cap):
        sp = np.zeros((max(cap, 1), 2), dtype=np.uint32)
        rg = np.zeros((max(cap, 1), 2), dtype=np.uint64)
        st = np.zeros(max(cap, 1), dtype=np.uint8)
        rc = L.debwt_fm_mems(fm._h, buf, api._p64(o), n, min_len, flags, api._p64(moff), sp.ctypes.data_as(u32p),
                             api._p64(rg), st.ctypes.data_as(u8p), cap)
        return rc, sp, rg, st

    assert call(offs, 0, 0, 10)[0] == -1
    assert call(offs, 1, 2, 10)[0] == -1
    assert call(offs, 1, 4, 10)[0] == -1
    bad = offs.copy()
    bad[3] = bad[4] + 1
    assert call(bad, 1, 0, 10)[0] == -1
    with pytest.raises(api.DebwtError) as e:
        fm.mems(["ACGT"], min_len=0)
    assert e.value.code == -1
    moff[:] = 0
    rc, *_ = call(offs, 1, 1, 1)
    total = int(moff[-1])
    assert rc == -5 and total > 1
    first = moff.copy()
    rc, sp, rg, st = call(offs, 1, 1, total)
    assert rc == 0 and np.array_equal(moff, first)
    res = fm.mems(pats, min_len=1, strands="both")
    assert np.array_equal(res.offsets, moff) and np.array_equal(res.spans, sp) and np.array_equal(res.ranges, rg)
    assert np.array_equal(res.strands, st)
    empty = fm.mems([], min_len=1)
    assert len(empty) == 0 and len(empty.spans) == 0
    fm.close()


def test_index_from_files(api):
    entry = entry_named("lowercase_3x2500")
    recs = golden_records(entry)
    text, _ = text_of(recs)
    words, hrows, drow = golden_outputs(entry)
    own = index_of(api, recs, s=4)
    opened = api.FMIndex.open(words, len(text), hrows, drow, own.samples(), sa_sample=4)
    pats = brute_patterns(rec_strings(recs), np.random.default_rng(41))
    a = own.mems(pats, min_len=1, strands="both")
    b = opened.mems(pats, min_len=1, strands="both")
    for k in ("offsets", "spans", "ranges", "strands"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert [x.tolist() for x in a.locate()] == [x.tolist() for x in b.locate()]
    own.close(); opened.close()


def test_scale_20mbp(api, monkeypatch):
    from debwt_amd import synth
    recs = synth.pan_genome(5_000_000, 4)
    strs = rec_strings(recs)
    fm = index_of(api, recs, s=16)
    rng = np.random.default_rng(43)
    reads, exact = [], []
    while len(reads) < 10_000:
        r = strs[int(rng.integers(0, len(strs)))]
        a = int(rng.integers(0, len(r) - 150))
        s = list(r[a:a + 150])
        k = int(rng.integers(0, 5))
        for _ in range(k):
            s[int(rng.integers(0, 150))] = "ACGT"[int(rng.integers(0, 4))]
        exact.append(k == 0)
        reads.append("".join(s))
    monkeypatch.setenv("DEBWT_FM_MEM_SLOTS", "400000")
    res = fm.mems(reads, min_len=1, strands="both")
    assert fm.mems_stats()["batches"] > 1
    monkeypatch.delenv("DEBWT_FM_MEM_SLOTS")
    assert np.array_equal(res.spans, fm.mems(reads, min_len=1, strands="both").spans)
    occ, gone, checks = [], [], []
    for i, p in enumerate(reads):
        m = len(p)
        sp, _, st = res.hits(i)
        for strand in (0, 1):
            q = p if strand == 0 else revcomp(p)
            mm = [(int(a), int(b)) if strand == 0 else (m - int(b), m - int(a)) for (a, b) in sp[st == strand].tolist()]
            mm.sort()
            assert all(x[0] < y[0] and x[1] < y[1] for x, y in zip(mm, mm[1:]))
            for a, b in mm:
                occ.append(q[a:b])
                if a > 0:
                    gone.append(q[a - 1:b])
                if b < m:
                    gone.append(q[a:b + 1])
            if i < 1500:                                      # s(e) from the MEMs: the first MEM ending at or after e
                j = 0
                for e in range(m):
                    while j < len(mm) and mm[j][1] <= e:
                        j += 1
                    s = mm[j][0] if j < len(mm) else e + 1
                    if s <= e:
                        checks.append((q[s:e + 1], True))
                        if s > 0:
                            checks.append((q[s - 1:e + 1], False))
                    else:
                        checks.append((q[e], False))
        if exact[i]:
            assert (0, 0, 150) in triples(res, i), i
            assert [t for t in triples(res, i) if t[0] == 0] == [(0, 0, 150)]
    assert np.all(fm.count(occ) > 0)
    assert np.all(fm.count(gone) == 0)
    cnt = fm.count([w for w, _ in checks])
    want = np.array([ok for _, ok in checks])
    assert np.array_equal(cnt > 0, want)
    long_reads = []                                           # longer than search allows
    for _ in range(40):
        r = strs[int(rng.integers(0, len(strs)))]
        a = int(rng.integers(0, len(r) - 2000))
        long_reads.append(r[a:a + 2000])
    lr = fm.mems(long_reads, min_len=19)
    for i in range(len(long_reads)):
        assert triples(lr, i) == [(0, 0, 2000)]
    fm.close()
