"""Gapped extension and the read mapper (debwt_fm_attach_text, debwt_fm_extend, debwt_fm_map).  The reference is the
recurrence of include/debwt_hip.h written out literally in Python over the records (class RefDP); every returned
alignment is checked to be valid and optimal without assuming a tie rule.  Then batching, the score-only variant, errors
and the capacity protocol, an index opened from files with a host text, and the mapper: exact conditions on golden
reads, and sensitivity on a collection without repeated 19-mers, where every read has to come back."""
import ctypes

import numpy as np
import pytest

from conftest import golden_outputs, golden_records
from test_fm_index_gpu import text_of
from test_fm_mems_gpu import rec_strings, revcomp
from test_fm_search_gpu import entry_named

pytestmark = pytest.mark.gpu
NEG = -10 ** 9
SCORINGS = [(1, 4, 6, 1), (2, 3, 0, 2)]
BANDS = [0, 1, 7, 16, 63]


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def index_with_text(api, recs, s=8):
    d = api.DeBWT(k=32)
    d.load_records(recs)
    d.build()
    fm = d.fm_index(sa_sample=s)
    fm.attach_text(d)
    d.close()
    return fm


class RefDP:
    """the definition, cell by cell: records joined by one separator each, record r's bases at [rs[r], re[r])"""

    def __init__(self, recs):
        self.strs = rec_strings(recs)
        self.text = "#".join(self.strs) + "$"
        self.rs, o = [], 0
        for s in self.strs:
            self.rs.append(o)
            o += len(s) + 1
        self.re = [a + len(s) for a, s in zip(self.rs, self.strs)]

    @staticmethod
    def query(p, strand):
        return (p if strand == 0 else revcomp(p)).upper()

    def allowed(self, m, i, t, diag, rec, w):
        return 0 <= i < m and self.rs[rec] <= t < self.re[rec] and abs(t - i - diag) <= w

    def sub(self, q, i, t, sc):
        return sc[0] if q[i] in "ACGT" and q[i] == self.text[t] else -sc[1]

    def score(self, p, strand, diag, rec, w, sc):
        return self.score_end(p, strand, diag, rec, w, sc)[0]

    def score_end(self, p, strand, diag, rec, w, sc):
        """(score, end row, end text position): the largest H, then the smallest row, then the smallest text position"""
        q = self.query(p, strand)
        m, (a, b, o, e) = len(q), sc
        H, E, F = {}, {}, {}
        best, bi, bt = 0, 0, 0
        for i in range(m):
            for t in range(max(self.rs[rec], i + diag - w), min(self.re[rec], i + diag + w + 1)):
                ev = max(H.get((i, t - 1), NEG) - o - e, E.get((i, t - 1), NEG) - e)
                fv = max(H.get((i - 1, t), NEG) - o - e, F.get((i - 1, t), NEG) - e)
                s = self.sub(q, i, t, sc)
                hv = max(0 + s, H.get((i - 1, t - 1), NEG) + s, ev, fv)
                H[(i, t)], E[(i, t)], F[(i, t)] = hv, ev, fv
                if hv > best:                                             # rows ascend, then text positions
                    best, bi, bt = hv, i, t
        return best, bi, bt

    def check(self, p, job, w, sc, score, qbeg, qend, tbeg, tend, edits, ops):
        """a valid alignment of score `score`: lengths, first and last op M, every visited cell allowed, re-scored, edits"""
        _, strand, diag, rec = job
        q = self.query(p, strand)
        m = len(q)
        if score == 0:
            assert (qbeg, qend, tbeg, tend, edits, len(ops)) == (0, 0, 0, 0, 0, 0)
            return
        assert score > 0 and len(ops) > 0
        kinds = [int(x) & 15 for x in ops]
        lens = [int(x) >> 4 for x in ops]
        assert all(k in (0, 1, 2) for k in kinds) and all(n > 0 for n in lens)
        assert all(k1 != k2 for k1, k2 in zip(kinds, kinds[1:])), "adjacent ops of one kind"
        assert kinds[0] == 0 and kinds[-1] == 0
        assert sum(n for k, n in zip(kinds, lens) if k in (0, 1)) == qend - qbeg
        assert sum(n for k, n in zip(kinds, lens) if k in (0, 2)) == tend - tbeg
        i, t, total, ed = qbeg, tbeg, 0, 0
        for k, n in zip(kinds, lens):
            if k == 0:
                for _ in range(n):
                    assert self.allowed(m, i, t, diag, rec, w), (job, i, t)
                    s = self.sub(q, i, t, sc)
                    total += s
                    ed += s < 0
                    i += 1
                    t += 1
            else:
                total -= sc[2] + n * sc[3]
                ed += n
                for _ in range(n):
                    if k == 1:
                        i += 1
                    else:
                        t += 1
                    assert self.allowed(m, i - 1, t - 1, diag, rec, w), (job, i, t)   # last query index / text position consumed
        assert (i, t) == (qend, tend)
        assert total == score, (job, total, score)
        assert ed == edits, (job, ed, edits)


def mutated_reads(R, rng, count, lo=8, hi=150):
    """(pattern, strand, record, true diagonal, edits made): reads cut from the records with 0-4 substitutions, insertions, deletions
    and N's, half of them given as their reverse complement"""
    out = []
    recs = [k for k, s in enumerate(R.strs) if len(s) >= 40]
    for n in range(count):
        rec = recs[int(rng.integers(0, len(recs)))]
        r = R.strs[rec]
        L = int(rng.integers(lo, min(len(r), hi) + 1))
        where = n % 5
        a = 0 if where == 0 else len(r) - L if where == 1 else int(rng.integers(0, len(r) - L + 1))
        s = list(r[a:a + L])
        nedit = int(rng.integers(0, 5))
        for _ in range(nedit):
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
        strand = int(rng.integers(0, 2))
        if strand:
            p = revcomp(p)
        if rng.random() < 0.2:
            p = p.lower()
        out.append((p, strand, rec, R.rs[rec] + a, nedit))
    return out


def jobs_for(R, reads, rng, w):
    """true loci with the diagonal off by up to w + 3, bands that leave the record or miss it, m = 1"""
    pats, jobs = [], []
    for p, strand, rec, diag, _ in reads:
        pats.append(p)
        k = len(pats) - 1
        jobs.append((k, strand, diag + int(rng.integers(-(w + 3), w + 4)), rec))
        if k % 4 == 0:
            jobs.append((k, 1 - strand, diag, rec))                       # the wrong strand: whatever aligns by chance
    m = len(pats[0])
    for rec in (0, len(R.strs) - 1):
        rs, re = R.rs[rec], R.re[rec]
        other = (rec + 1) % len(R.strs)
        jobs += [(0, reads[0][1], rs - m + 3, rec), (0, reads[0][1], re - 3, rec),           # the band leaves the record
                 (0, 0, rs - m - w - 1, rec), (0, 1, re + w, rec), (0, 0, rs - m - w, rec), (0, 1, re + w - 1, rec),
                 (0, 0, re + w + 40, rec), (0, 0, -(2 ** 62), rec), (0, 1, 2 ** 62, rec),      # wholly outside: score 0
                 (0, reads[0][1], reads[0][3], other)]                                       # another record's text
    for ch in "ACGTN":
        pats.append(ch)
        k = len(pats) - 1
        for rec in range(min(len(R.strs), 2)):
            jobs += [(k, 0, R.rs[rec], rec), (k, 1, R.re[rec] - 1, rec), (k, 0, R.rs[rec] + 5 - w, rec)]
    return pats, jobs


def check_all(R, pats, jobs, w, sc, res):
    assert len(res) == len(jobs)
    for j, job in enumerate(jobs):
        p = pats[job[0]]
        want, ei, et = R.score_end(p, job[1], job[2], job[3], w, sc)
        assert int(res.score[j]) == want, (job, w, sc, int(res.score[j]), want)
        if want:
            assert (int(res.qend[j]) - 1, int(res.tend[j]) - 1) == (ei, et), (job, w, sc)
        R.check(p, job, w, sc, want, int(res.qbeg[j]), int(res.qend[j]), int(res.tbeg[j]), int(res.tend[j]),
                int(res.edits[j]), res.ops(j))


@pytest.mark.parametrize("name", ["shared_ends_duplicates", "lowercase_3x2500", "homopolymers_tandem"])
def test_extension_against_definition(api, name):
    recs = golden_records(entry_named(name))
    R = RefDP(recs)
    fm = index_with_text(api, recs)
    total = 0
    for n, w in enumerate(BANDS):
        for sc in SCORINGS:
            rng = np.random.default_rng(1000 * n + sc[0])
            reads = mutated_reads(R, rng, 16 if w == 63 else 30, hi=100 if w == 63 else 150)
            pats, jobs = jobs_for(R, reads, rng, w)
            res = fm.extend(pats, jobs, scoring=sc, band=w)
            check_all(R, pats, jobs, w, sc, res)
            st = fm.extend_stats()
            assert st["jobs"] == len(jobs) and st["cells"] > 0 and st["wave_steps"] > 0
            assert st["cells"] <= 64 * st["wave_steps"]
            total += len(jobs)
            # true loci at the true diagonal with a band that holds their (at most 4) indel bases: the read's own
            # alignment is among the candidates, and an edit costs it at most one match and one mismatch or 1-base gap
            for p, strand, rec, diag, _ in reads:
                if w >= 7:
                    r1 = fm.extend([p], [(0, strand, diag, rec)], scoring=sc, band=w)
                    assert int(r1.score[0]) >= sc[0] * len(p) - 4 * (sc[0] + max(sc[1], sc[2] + sc[3])), (p, w, sc)
    assert total > 300
    fm.close()


def test_batching_and_score_only(api, monkeypatch):
    recs = golden_records(entry_named("pan_4x20k"))
    R = RefDP(recs)
    fm = index_with_text(api, recs)
    rng = np.random.default_rng(77)
    for w, sc in ((16, SCORINGS[0]), (5, SCORINGS[1]), (40, SCORINGS[0])):
        reads = mutated_reads(R, rng, 40)
        pats, jobs = jobs_for(R, reads, rng, w)
        long_read = R.strs[1][100:3100]                                   # one job far longer than the others
        pats.append(long_read[:1500] + long_read[1503:])
        jobs.insert(7, (len(pats) - 1, 0, R.rs[1] + 100, 1))
        monkeypatch.delenv("DEBWT_FM_EXTEND_BYTES", raising=False)
        ref = fm.extend(pats, jobs, scoring=sc, band=w)
        assert fm.extend_stats()["batches"] == 1
        assert int(ref.score[7]) == sc[0] * 2997 - sc[2] - 3 * sc[3]         # all of it, with the 3 deleted bases as one gap
        R.check(pats[-1], jobs[7], w, sc, int(ref.score[7]), int(ref.qbeg[7]), int(ref.qend[7]), int(ref.tbeg[7]),
                int(ref.tend[7]), int(ref.edits[7]), ref.ops(7))
        assert (int(ref.qbeg[7]), int(ref.qend[7]), int(ref.edits[7])) == (0, 2997, 3)
        monkeypatch.setenv("DEBWT_FM_EXTEND_BYTES", "1")                  # every job alone
        one = fm.extend(pats, jobs, scoring=sc, band=w)
        st = fm.extend_stats()
        assert st["batches"] > 40 and st["batches"] <= len(jobs)
        monkeypatch.setenv("DEBWT_FM_EXTEND_BYTES", "20000")
        some = fm.extend(pats, jobs, scoring=sc, band=w)
        assert 1 < fm.extend_stats()["batches"] <= st["batches"]
        for other in (one, some):
            assert np.array_equal(ref.aln, other.aln) and np.array_equal(ref.offsets, other.offsets)
            assert np.array_equal(ref.cigars, other.cigars)
        monkeypatch.delenv("DEBWT_FM_EXTEND_BYTES")
        so = fm.extend(pats, jobs, scoring=sc, band=w, cigar=False)
        assert so.cigar(0) is None and fm.extend_stats()["scratch_bytes"] == 0
        assert np.array_equal(so.score, ref.score) and np.array_equal(so.qend, ref.qend) and np.array_equal(so.tend, ref.tend)
        assert not so.qbeg.any() and not so.tbeg.any() and not so.edits.any()
    fm.close()


def test_errors_and_protocol(api):
    from debwt_amd import _lib
    entry = entry_named("lowercase_3x2500")
    recs = golden_records(entry)
    R = RefDP(recs)
    d = api.DeBWT(k=32)
    d.load_records(recs)
    d.build()
    fm = d.fm_index(sa_sample=4)
    p = R.strs[0][10:70]
    job = (0, 0, R.rs[0] + 10, 0)
    for call in (lambda: fm.extend([p], [job]), lambda: fm.map([p])):     # no text attached
        with pytest.raises(api.DebwtError) as e:
            call()
        assert e.value.code == -4
    assert len(fm.mems([p])) == 1 and int(fm.count([p])[0]) >= 1          # the rest never needs it
    before = fm.info()["device_bytes"]
    # a wrong text: one base changed before a sampled suffix; a shifted record boundary
    words, n, sep = api.pack_records(recs)
    samples = fm.samples()
    seps = set(int(x) for x in sep)
    pos = next(int(x) - 1 for x in samples if int(x) > 0 and int(x) - 1 not in seps)
    bad = words.copy()
    bad[pos >> 5] ^= np.uint64(1) << np.uint64(2 * (31 - (pos & 31)))
    with pytest.raises(api.DebwtError) as e:
        fm.attach_text(words=bad, sep=sep)
    assert e.value.code == -1 and "sampled" in str(e.value)
    shifted = sep.copy()
    shifted[0] += 1
    with pytest.raises(api.DebwtError) as e:
        fm.attach_text(words=words, sep=shifted)
    assert e.value.code == -1 and "separator" in str(e.value)
    with pytest.raises(api.DebwtError):
        fm.extend([p], [job])                                             # a refused text is not attached
    other = api.DeBWT(k=32)
    other.load_records(recs[:2])
    with pytest.raises(api.DebwtError) as e:
        fm.attach_text(other)
    assert e.value.code == -1
    other.close()
    fm.attach_text(d)
    d.close()
    assert fm.info()["device_bytes"] >= before + n // 4
    ok = fm.extend([p], [job])
    assert int(ok.score[0]) == 60 and ok.cigar(0) == "60M" and int(ok.tbeg[0]) == R.rs[0] + 10
    for kw in (dict(band=64), dict(scoring=(1, 4, 6, 0)), dict(scoring=(0, 4, 6, 1)), dict(scoring=(1, 0, 6, 1)),
               dict(scoring=(256, 4, 6, 1)), dict(scoring=(1, 4, 256, 1)), dict(scoring=(1, 4, -1, 1))):
        with pytest.raises(api.DebwtError) as e:
            fm.extend([p], [job], **kw)
        assert e.value.code == -1, kw
    big = "ACGT" * 16384
    for pats, jb in (([""], (0, 0, 0, 0)), ([big], (0, 0, 0, 0)), ([p], (0, 0, 0, len(recs))), ([p], (1, 0, 0, 0)),
                     ([p], (0, 2, 0, 0))):
        with pytest.raises(api.DebwtError) as e:
            fm.extend(pats, [jb])
        assert e.value.code == -1, jb
    assert int(fm.extend([big[:65535]], [(0, 0, 0, 0)], band=3).score[0]) >= 0               # the longest pattern allowed
    assert len(fm.extend([p], [])) == 0
    # the capacity protocol: offsets and alignments first, then DEBWT_ERANGE
    rng = np.random.default_rng(5)
    pats, jobs = jobs_for(R, mutated_reads(R, rng, 20), rng, 16)
    ref = fm.extend(pats, jobs)
    total = len(ref.cigars)
    assert total > len(jobs) // 2
    L = _lib.lib()
    buf, offs = api._patterns(pats)
    ja = (_lib.DebwtFmJob * len(jobs))()
    for k, (a, s, dg, r) in enumerate(jobs):
        ja[k].pattern, ja[k].strand, ja[k].diag, ja[k].record = a, s, dg, r
    sc = _lib.DebwtFmScoring(1, 4, 6, 1)
    out = np.zeros(len(jobs), dtype=api._ALN_DTYPE)
    coff = np.zeros(len(jobs) + 1, dtype=np.uint64)
    cg = np.zeros(total, dtype=np.uint32)
    u32p, alnp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_lib.DebwtFmAln)

    def call(cap, cigar=True):
        return L.debwt_fm_extend(fm._h, buf, api._p64(offs), len(pats), ja, len(jobs), ctypes.byref(sc), 16,
                                 out.ctypes.data_as(alnp), api._p64(coff), cg.ctypes.data_as(u32p) if cigar else None, cap)

    assert call(total - 1) == -5
    assert np.array_equal(coff, ref.offsets) and np.array_equal(out, ref.aln)
    assert call(total, cigar=False) == -5
    assert call(total) == 0 and np.array_equal(cg, ref.cigars)
    fm.close()


def test_index_from_files_with_host_text(api):
    entry = entry_named("lowercase_3x2500")
    recs = golden_records(entry)
    R = RefDP(recs)
    text, _ = text_of(recs)
    words, hrows, drow = golden_outputs(entry)
    own = index_with_text(api, recs, s=4)
    opened = api.FMIndex.open(words, len(text), hrows, drow, own.samples(), sa_sample=4)
    tw, n, sep = api.pack_records(recs)
    assert n == len(text)
    opened.attach_text(words=tw, sep=sep)
    rng = np.random.default_rng(9)
    reads = mutated_reads(R, rng, 40)
    pats, jobs = jobs_for(R, reads, rng, 16)
    a, b = own.extend(pats, jobs), opened.extend(pats, jobs)
    assert np.array_equal(a.aln, b.aln) and np.array_equal(a.offsets, b.offsets) and np.array_equal(a.cigars, b.cigars)
    ma, mb = own.map(pats, min_len=12), opened.map(pats, min_len=12)
    assert np.array_equal(ma.hits, mb.hits) and np.array_equal(ma.cigars, mb.cigars)
    own.close(); opened.close()


def check_hits(R, pats, res, w, sc, min_score):
    """every mapped read: a valid alignment whose score is the reference DP of (read, strand, diag, w)"""
    from debwt_amd import api as A
    mapped = 0
    for i, p in enumerate(pats):
        fl = int(res.flags[i])
        assert int(res.pattern[i]) == i
        if fl & A.MAP_UNMAPPED:
            assert int(res.score[i]) == 0 and len(res.ops(i)) == 0 and int(res.mapq[i]) == 0
            assert bool(fl & A.MAP_TOO_LONG) == (len(p) > 65535)
            continue
        mapped += 1
        strand, rec, diag = fl & A.MAP_REVERSE, int(res.record[i]), int(res.diag[i])
        score = int(res.score[i])
        assert score >= min_score and 0 <= int(res.sub[i]) <= score
        assert int(res.mapq[i]) == 60 * (score - int(res.sub[i])) // score
        assert int(res.tbeg[i]) == R.rs[rec] + int(res.offset[i])
        assert score == R.score(p, strand, diag, rec, w, sc), (i, p)
        R.check(p, (i, strand, diag, rec), w, sc, score, int(res.qbeg[i]), int(res.qend[i]), int(res.tbeg[i]),
                int(res.tend[i]), int(res.edits[i]), res.ops(i))
    return mapped


@pytest.mark.parametrize("name", ["pan_4x20k", "shared_ends_duplicates"])
def test_mapper_exact_conditions(api, name):
    recs = golden_records(entry_named(name))
    R = RefDP(recs)
    fm = index_with_text(api, recs)
    rng = np.random.default_rng(123)
    reads = mutated_reads(R, rng, 60, lo=30, hi=150)
    pats = [r[0] for r in reads] + ["N" * 40, "", "ACGT", "".join("ACGT"[int(x)] for x in rng.integers(0, 4, 80))]
    res = fm.map(pats)
    st = fm.map_stats()
    assert st["reads"] == len(pats) and st["jobs"] == st["candidates"] and st["seeds"] >= st["candidates"]
    mapped = check_hits(R, pats, res, 16, (1, 4, 6, 1), 30)
    assert mapped == st["mapped"] == int(res.mapped.sum())
    for i, (p, _, _, _, nedit) in enumerate(reads):                       # an unedited read of 30 bases or more is one MEM
        if nedit == 0:
            assert res.mapped[i] and int(res.score[i]) == len(p) and res.cigar(i) == f"{len(p)}M", i
    assert sum(1 for r in reads if r[4] == 0) >= 3
    assert not res.mapped[len(reads):len(reads) + 3].any()
    for kw in (dict(min_len=12, band=8, scoring=(2, 3, 0, 2), min_score=20), dict(strands="forward", max_occ=2, max_cand=1)):
        r2 = fm.map(pats, **kw)
        check_hits(R, pats, r2, kw.get("band", 16), kw.get("scoring", (1, 4, 6, 1)), kw.get("min_score", 30))
        if kw.get("strands") == "forward":
            assert not (r2.flags & api.MAP_REVERSE).any()
    fm.close()


def random_collection(seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, 2500).astype(np.uint8) for _ in range(3)], rng


def kmers(s, k=19):
    return [s[i:i + k] for i in range(len(s) - k + 1)]


def edited_read(seg, rng):
    """seg with at most 4 edit events (substitution, 1-base indel, indel of up to 3 bases): the read, its error-free
    stretches as (start in the read, length), and the largest shift of its diagonal against the read's first base"""
    nev = int(rng.integers(0, 5))
    pos = sorted(int(x) for x in rng.choice(np.arange(1, len(seg) - 4), size=nev, replace=False))
    parts, stretches = [], []
    cur = rlen = run_start = shift = worst = 0              # next base of seg, read length so far, start of the stretch
    for c in pos:
        if c < cur:
            continue                                        # inside the deletion before it
        parts.append(seg[cur:c])
        rlen += c - cur
        stretches.append((run_start, rlen - run_start))
        kind = int(rng.integers(0, 3))
        L = 1 if kind < 2 else int(rng.integers(1, 4))
        if kind == 0:                                       # substitution by another base
            parts.append("ACGT"[("ACGT".index(seg[c]) + int(rng.integers(1, 4))) % 4])
            rlen += 1
            cur = c + 1
        elif rng.random() < 0.5:                            # insertion of L bases before c
            parts.append("".join("ACGT"[int(x)] for x in rng.integers(0, 4, L)))
            rlen += L
            cur = c
            shift -= L
        else:                                               # deletion of L bases from c
            cur = c + L
            shift += L
        worst = max(worst, abs(shift))
        run_start = rlen
    parts.append(seg[cur:])
    rlen += len(seg) - cur
    stretches.append((run_start, rlen - run_start))
    read = "".join(parts)
    assert len(read) == rlen
    return read, stretches, worst


def test_mapper_sensitivity(api):
    recs, rng = random_collection(20240607)
    R = RefDP(recs)
    both = [s for r in R.strs for s in (r, revcomp(r))]
    all19 = [k for s in both for k in kmers(s)]
    assert len(set(all19)) == len(all19), "the collection repeats a 19-mer"   # a condition on the input, not luck
    where = {}
    for rec, r in enumerate(R.strs):
        for o, k in enumerate(kmers(r)):
            where[k] = (rec, o)
    reads, truth = [], []
    while len(reads) < 200:
        rec = int(rng.integers(0, 3))
        a = int(rng.integers(0, 2400))
        seg = R.strs[rec][a:a + 100]
        read, stretches, worst = edited_read(seg, rng)
        if max(n for _, n in stretches) < 20:
            continue                                                      # redrawn: a seed of 19 needs a stretch
        strand = len(reads) % 2
        assert len(read) >= 88 and worst <= 12
        # the longest error-free stretch is where the generator says it is, at the true locus within the indel shift
        s0, n0 = max(stretches, key=lambda x: x[1])
        assert n0 >= 20
        hit = R.strs[rec].find(read[s0:s0 + n0])
        assert hit >= 0 and abs((hit - s0) - a) <= 12
        reads.append(revcomp(read) if strand else read)
        truth.append((strand, rec, R.rs[rec] + a))
    fm = index_with_text(api, recs, s=4)
    res = fm.map(reads)                                                   # the defaults: min_len 19, w 16
    sc, w = (1, 4, 6, 1), 16
    for i, (read, (strand, rec, diag)) in enumerate(zip(reads, truth)):
        assert res.mapped[i], i
        assert (int(res.strand[i]), int(res.record[i])) == (strand, rec), i
        assert int(res.score[i]) >= R.score(read, strand, diag, rec, w, sc), i
        assert abs(int(res.tbeg[i]) - int(res.qbeg[i]) - diag) <= w, i
        # a second exact 19-mer of the read or its reverse complement away from the true locus?
        elsewhere = False
        for st, q in ((0, read), (1, revcomp(read))):
            for x, k in enumerate(kmers(q)):
                for s2, kk in ((0, k), (1, revcomp(k))):
                    if kk not in where:
                        continue
                    r2, o2 = where[kk]
                    tstrand = st ^ s2                                       # strand of the read that reads this text forward
                    xq = x if s2 == 0 else len(q) - 19 - x                  # in the coordinates of that strand's query
                    if not (tstrand == strand and r2 == rec and abs(R.rs[r2] + o2 - xq - diag) <= 12):
                        elsewhere = True
        if not elsewhere:
            assert int(res.mapq[i]) == 60, i
    check_hits(R, reads, res, w, sc, 30)
    fm.close()
    # a region planted twice: a read from it has two equal loci
    recs2, rng2 = random_collection(99)
    recs2[2][700:1700] = recs2[0][300:1300]
    R2 = RefDP(recs2)
    fm2 = index_with_text(api, recs2, s=4)
    twice = [R2.strs[0][700:800], revcomp(R2.strs[0][1000:1100]), R2.strs[1][500:600]]
    for k in kmers(twice[2]):                                             # the third read's 19-mers occur once
        assert R2.text.count(k) == 1 and revcomp(k) not in R2.text
    r2 = fm2.map(twice)
    assert r2.mapped.all() and [int(x) for x in r2.mapq] == [0, 0, 60]
    assert [int(x) for x in r2.score] == [100, 100, 100] and [int(x) for x in r2.sub] == [100, 100, 0]
    assert (int(r2.record[0]), int(r2.offset[0])) == (0, 700) and r2.cigar(0) == "100M"
    fm2.close()
