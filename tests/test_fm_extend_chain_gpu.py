"""Extension along a chain and the chained mapper (debwt_fm_extend_chain, debwt_fm_map_chained).  The reference is the
recurrence of include/debwt_hip.h over the allowed cells of a chain, written out literally in Python
(fm_chain_ref.chain_dp): score and end cell are compared, every returned alignment is re-scored and checked to stay inside
the allowed cells.  A job with one anchor must equal debwt_fm_extend bit for bit, up to the length limit.  Then batching,
the score-only variant, errors and the capacity protocol, and the mapper: exact conditions on golden reads, and reads with
one-sided indels that a fixed band loses and a band along the chain keeps."""
import ctypes

import numpy as np
import pytest

from conftest import golden_records
from fm_chain_ref import chain_dp, chain_dp_rows, drift_reads
from test_fm_extend_gpu import RefDP, index_with_text, jobs_for, mutated_reads
from test_fm_search_gpu import entry_named

pytestmark = pytest.mark.gpu
SCORINGS = [(1, 4, 6, 1), (2, 3, 0, 2)]
BANDS = [0, 1, 7, 15, 16, 31, 32, 63]


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


class ChainRef(RefDP):
    """RefDP with the allowed cells of a chain: where RefDP takes a diagonal, this takes the tuple of (qbeg, diag)"""

    def allowed(self, m, i, t, anchors, rec, w):
        c = anchors[0][1]
        for q, d in anchors:
            if q <= i:
                c = d
        return 0 <= i < m and self.rs[rec] <= t < self.re[rec] and abs(t - i - c) <= w

    def dp(self, p, strand, rec, anchors, w, sc):
        return chain_dp(self.query(p, strand), self.text, self.rs[rec], self.re[rec], anchors, w, sc)


def flatten(chains):
    """[(pattern, strand, record, [(qbeg, diag)])] -> the job rows and anchor rows of FMIndex.extend_chain"""
    jobs, anchors = [], []
    for p, s, r, an in chains:
        jobs.append((p, s, r, len(anchors), len(an)))
        anchors += an
    return jobs, anchors


def random_chain(rng, m, diag, w, n=None, steps=None):
    n = min(int(rng.integers(1, 9)) if n is None else n, m)
    qs = sorted(int(x) for x in rng.choice(np.arange(m), size=n, replace=False))
    how = int(rng.integers(0, 4))
    if how == 0:
        qs[0] = 0
    elif how == 1:
        qs[-1] = m - 1
    qs = sorted(set(qs))
    an, d = [], diag
    for x, q in enumerate(qs):
        if x:
            d += int(rng.choice(steps if steps is not None else [w, -w, 1, -1, 0] if w else [0]))
        an.append((q, d))
    return an


def chains_for(R, reads, rng, w):
    """chains through the true loci with a start off by up to w + 3, one-way chains that drift more than 2w, chains at
    and beyond both ends of a record, far outside it, and m = 1"""
    pats, chains = [], []
    for n, (p, strand, rec, diag, _) in enumerate(reads):
        pats.append(p)
        k = len(pats) - 1
        d0 = diag + int(rng.integers(-(w + 3), w + 4))
        chains.append((k, strand, rec, random_chain(rng, len(p), d0, w)))
        if n % 4 == 0:
            chains.append((k, 1 - strand, rec, random_chain(rng, len(p), diag, w)))
        if n % 5 == 0 and len(p) >= 8 and w:
            one_way = random_chain(rng, len(p), diag, w, n=8, steps=[w] if n % 10 else [-w])
            assert abs(one_way[-1][1] - one_way[0][1]) > 2 * w
            chains.append((k, strand, rec, one_way))
    m = len(pats[0])
    for rec in (0, len(R.strs) - 1):
        rs, re = R.rs[rec], R.re[rec]
        for d in (rs - m + 3, re - 3, rs - m - w, re + w - 1):                          # the band leaves the record
            chains.append((0, reads[0][1], rec, random_chain(rng, m, d, w)))
        for d in (rs - m - w - 1 - 8 * w, re + w + 8 * w, re + 5000, -(2 ** 62), 2 ** 62):   # wholly outside: score 0
            chains.append((0, 0, rec, random_chain(rng, m, d, w)))
    for ch in "ACGTN":
        pats.append(ch)
        k = len(pats) - 1
        chains += [(k, 0, 0, [(0, R.rs[0])]), (k, 1, 0, [(0, R.re[0] - 1)]), (k, 0, 0, [(0, R.rs[0] + 5 - w)])]
    return pats, chains


def check_chains(R, pats, chains, w, sc, res):
    assert len(res) == len(chains)
    for j, (k, strand, rec, an) in enumerate(chains):
        p = pats[k]
        want, ei, et = R.dp(p, strand, rec, an, w, sc)
        assert int(res.score[j]) == want, (chains[j], w, sc, int(res.score[j]), want)
        if want:
            assert (int(res.qend[j]) - 1, int(res.tend[j]) - 1) == (ei, et), (chains[j], w, sc)
        R.check(p, (k, strand, tuple(an), rec), w, sc, want, int(res.qbeg[j]), int(res.qend[j]), int(res.tbeg[j]),
                int(res.tend[j]), int(res.edits[j]), res.ops(j))


@pytest.mark.parametrize("name", ["shared_ends_duplicates", "lowercase_3x2500", "homopolymers_tandem"])
def test_chain_extension_against_definition(api, name):
    recs = golden_records(entry_named(name))
    R = ChainRef(recs)
    fm = index_with_text(api, recs)
    total = 0
    for n, w in enumerate(BANDS):
        sc = SCORINGS[n % 2]
        rng = np.random.default_rng(500 * n + 7)
        reads = mutated_reads(R, rng, 10 if w >= 32 else 16, hi=90 if w >= 32 else 150)
        if w in (15, 16):
            # up to 300 bases; mutated_reads draws from every record of 40 bases or more, so no longer than the shortest
            reads += mutated_reads(R, rng, 2, lo=min(250, min(len(s) for s in R.strs if len(s) >= 40)), hi=300)
        pats, chains = chains_for(R, reads, rng, w)
        jobs, anchors = flatten(chains)
        res = fm.extend_chain(pats, jobs, anchors, scoring=sc, band=w)
        check_chains(R, pats, chains, w, sc, res)
        st = fm.extend_stats()
        assert st["jobs"] == len(jobs) and st["cells"] > 0 and st["wave_steps"] > 0
        assert st["cells"] <= 64 * (1 if w < 32 else 2) * st["wave_steps"]
        so = fm.extend_chain(pats, jobs, anchors, scoring=sc, band=w, cigar=False)
        assert np.array_equal(so.score, res.score) and np.array_equal(so.qend, res.qend) and np.array_equal(so.tend, res.tend)
        assert not so.qbeg.any() and not so.tbeg.any() and not so.edits.any()
        total += len(jobs)
    assert total > 250
    fm.close()


def planted_chain(R, rec, start, rng, nseg, seg, w, sign=0):
    """a query cut from record `rec` at `start` in nseg pieces of `seg` bases with an indel of up to w bases between two
    pieces (sign +1: deletions from the read only, -1: insertions only), and the chain that follows it"""
    parts, an, t, q = [], [], start, 0
    for x in range(nseg):
        an.append((q, R.rs[rec] + t - q))
        parts.append(R.strs[rec][t:t + seg])
        t += seg
        q += seg
        n = int(rng.integers(1, w + 1))
        s = sign or (1 if rng.random() < 0.5 else -1)
        if x + 1 < nseg:
            if s > 0:
                t += n
            else:
                parts.append("".join("ACGT"[int(c)] for c in rng.integers(0, 4, n)))
                q += n
    return "".join(parts), an


def test_long_job_with_forty_anchors(api):
    recs = golden_records(entry_named("pan_4x20k"))
    R = ChainRef(recs)
    fm = index_with_text(api, recs)
    rng = np.random.default_rng(40)
    sc, w = (1, 4, 6, 1), 63
    p, an = planted_chain(R, 1, 200, rng, 40, 72, w)
    assert 2800 <= len(p) <= 4200 and len(an) == 40
    for strand, pat in ((1, "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(p))),):
        chains = [(0, strand, 1, an)]
        jobs, anchors = flatten(chains)
        res = fm.extend_chain([pat], jobs, anchors, scoring=sc, band=w)
        check_chains(R, [pat], chains, w, sc, res)
        assert int(res.qend[0]) - int(res.qbeg[0]) >= len(p) - 80          # the planted alignment, end to end
    fm.close()


def test_one_anchor_equals_extend(api):
    recs = golden_records(entry_named("pan_4x20k"))
    R = RefDP(recs)
    fm = index_with_text(api, recs)
    total = 0
    for n, w in enumerate((0, 7, 16, 31, 32, 63)):
        rng = np.random.default_rng(900 + n)
        pats, jobs = jobs_for(R, mutated_reads(R, rng, 60), rng, w)
        cj = [(p, s, r, k, 1) for k, (p, s, d, r) in enumerate(jobs)]
        ca = [(0 if k % 3 else min(5, len(pats[j[0]]) - 1), j[2]) for k, j in enumerate(jobs)]   # where the anchor starts does not matter
        sc = SCORINGS[n % 2]
        for cigar in (True, False):
            a = fm.extend(pats, jobs, scoring=sc, band=w, cigar=cigar)
            b = fm.extend_chain(pats, cj, ca, scoring=sc, band=w, cigar=cigar)
            assert np.array_equal(a.aln, b.aln), w
            if cigar:
                assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.cigars, b.cigars), w
        total += len(jobs)
    assert total > 300
    # the length limit: the whole of record 0, then bases that match nothing in reach
    rng = np.random.default_rng(65535)
    big = R.strs[0] + "".join("ACGT"[int(c)] for c in rng.integers(0, 4, 65535 - len(R.strs[0])))
    big = big[:7000] + big[7003:9000] + "ACG" + big[9000:]                  # a 3-base deletion and a 3-base insertion
    assert len(big) == 65535
    for w in (63, 16):
        for cigar in (True, False):
            a = fm.extend([big], [(0, 0, R.rs[0], 0)], band=w, cigar=cigar)
            b = fm.extend_chain([big], [(0, 0, 0, 0, 1)], [(0, R.rs[0])], band=w, cigar=cigar)
            assert np.array_equal(a.aln, b.aln) and int(a.score[0]) > 19000
            if cigar:
                assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.cigars, b.cigars) and len(a.cigars) >= 5
    fm.close()


def test_length_limit_with_fifty_anchors(api):
    """m = 65535, 50 anchors, every step +62: a drift of 3038 diagonals, score-only, against the numpy row form"""
    recs = golden_records(entry_named("pan_4x20k"))
    R = ChainRef(recs)
    fm = index_with_text(api, recs)
    rng = np.random.default_rng(50)
    sc, w, seg = (1, 4, 6, 1), 63, 330
    parts, an = [], []
    for a in range(50):
        parts.append(R.strs[2][a * (seg + 62):a * (seg + 62) + seg])
        an.append((a * seg, R.rs[2] + 62 * a))
    p = "".join(parts)
    p += "".join("ACGT"[int(c)] for c in rng.integers(0, 4, 65535 - len(p)))
    assert len(p) == 65535 and an[-1][1] - an[0][1] > 3000
    res = fm.extend_chain([p], [(0, 0, 2, 0, 50)], an, scoring=sc, band=w, cigar=False)
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    want = chain_dp_rows([code[c] for c in p], [code.get(c, 5) for c in R.text], R.rs[2], R.re[2], an, w, sc)
    assert int(res.score[0]) == want
    assert want >= 50 * seg - 49 * (6 + 62)                                 # the planted alignment is among the paths
    # the same chain with its traceback ends where the score-only run ends; its path is valid and re-scores
    tr = fm.extend_chain([p], [(0, 0, 2, 0, 50)], an, scoring=sc, band=w)
    assert (int(tr.score[0]), int(tr.qend[0]), int(tr.tend[0])) == (want, int(res.qend[0]), int(res.tend[0]))
    R.check(p, (0, 0, tuple(an), 2), w, sc, want, int(tr.qbeg[0]), int(tr.qend[0]), int(tr.tbeg[0]), int(tr.tend[0]),
            int(tr.edits[0]), tr.ops(0))
    fm.close()


def test_batching_and_score_only(api, monkeypatch):
    recs = golden_records(entry_named("pan_4x20k"))
    R = ChainRef(recs)
    fm = index_with_text(api, recs)
    rng = np.random.default_rng(78)
    for w, sc in ((16, SCORINGS[0]), (5, SCORINGS[1]), (40, SCORINGS[0])):
        pats, chains = chains_for(R, mutated_reads(R, rng, 40), rng, w)
        p, an = planted_chain(R, 1, 100, rng, 30, 100, w)                  # one job far longer than the others
        pats.append(p)
        chains.insert(7, (len(pats) - 1, 0, 1, an))
        jobs, anchors = flatten(chains)
        monkeypatch.delenv("DEBWT_FM_EXTEND_BYTES", raising=False)
        ref = fm.extend_chain(pats, jobs, anchors, scoring=sc, band=w)
        assert fm.extend_stats()["batches"] == 1
        assert int(ref.qend[7]) - int(ref.qbeg[7]) >= len(p) - 2 * w
        monkeypatch.setenv("DEBWT_FM_EXTEND_BYTES", "1")                  # every job alone
        one = fm.extend_chain(pats, jobs, anchors, scoring=sc, band=w)
        st = fm.extend_stats()
        assert st["batches"] > 40 and st["batches"] <= len(jobs)
        monkeypatch.setenv("DEBWT_FM_EXTEND_BYTES", "20000")
        some = fm.extend_chain(pats, jobs, anchors, scoring=sc, band=w)
        assert 1 < fm.extend_stats()["batches"] <= st["batches"]
        for other in (one, some):
            assert np.array_equal(ref.aln, other.aln) and np.array_equal(ref.offsets, other.offsets)
            assert np.array_equal(ref.cigars, other.cigars)
        monkeypatch.delenv("DEBWT_FM_EXTEND_BYTES")
        so = fm.extend_chain(pats, jobs, anchors, scoring=sc, band=w, cigar=False)
        assert so.cigar(0) is None and fm.extend_stats()["scratch_bytes"] == 0
        assert np.array_equal(so.score, ref.score) and np.array_equal(so.qend, ref.qend) and np.array_equal(so.tend, ref.tend)
    fm.close()


def test_errors_and_protocol(api):
    from debwt_amd import _lib
    recs = golden_records(entry_named("lowercase_3x2500"))
    R = ChainRef(recs)
    d = api.DeBWT(k=32)
    d.load_records(recs)
    d.build()
    fm = d.fm_index(sa_sample=4)
    p = R.strs[0][10:70]
    an = [(0, R.rs[0] + 10), (30, R.rs[0] + 12)]
    for call in (lambda: fm.extend_chain([p], [(0, 0, 0, 0, 2)], an), lambda: fm.map_chained([p])):   # no text attached
        with pytest.raises(api.DebwtError) as e:
            call()
        assert e.value.code == -4
    fm.attach_text(d)
    d.close()
    ok = fm.extend_chain([p], [(0, 0, 0, 0, 2)], an)
    assert int(ok.score[0]) == 60 and ok.cigar(0) == "60M"
    bad = [
        ([(0, 0, 0, 0, 0)], an, {}),                                      # no anchor
        ([(0, 0, 0, 1, 2)], an, {}), ([(0, 0, 0, 3, 1)], an, {}), ([(0, 0, 0, 0, 3)], an, {}),   # anchors out of range
        ([(0, 0, 0, 0, 2)], [(30, 5), (30, 5)], {}), ([(0, 0, 0, 0, 2)], [(30, 5), (29, 5)], {}),   # qbeg not increasing
        ([(0, 0, 0, 0, 2)], [(0, 5), (60, 5)], {}), ([(0, 0, 0, 0, 1)], [(60, 5)], {}),          # qbeg >= m
        ([(0, 0, 0, 0, 2)], [(0, 5), (30, 22)], {}), ([(0, 0, 0, 0, 2)], [(0, 5), (30, -12)], {}),   # a step above the band
        ([(0, 0, 0, 0, 2)], [(0, -(2 ** 62)), (30, 2 ** 62)], {}),
        ([(0, 0, 0, 0, 2)], an, dict(band=1)), ([(0, 0, 0, 0, 2)], an, dict(band=64)),
        ([(0, 0, 0, 0, 2)], an, dict(scoring=(1, 4, 6, 0))), ([(0, 0, 0, 0, 2)], an, dict(scoring=(1, 4, 256, 1))),
        ([(1, 0, 0, 0, 2)], an, {}), ([(0, 2, 0, 0, 2)], an, {}), ([(0, 0, len(recs), 0, 2)], an, {}),
    ]
    for jobs, anchors, kw in bad:
        with pytest.raises(api.DebwtError) as e:
            fm.extend_chain([p], jobs, anchors, **kw)
        assert e.value.code == -1, (jobs, anchors, kw)
    for pats in ([""], ["ACGT" * 16384]):
        with pytest.raises(api.DebwtError) as e:
            fm.extend_chain(pats, [(0, 0, 0, 0, 1)], [(0, 0)])
        assert e.value.code == -1
    assert int(fm.extend_chain([p], [(0, 0, 0, 0, 2)], [(0, 5), (30, 21)]).score[0]) >= 0      # a step of exactly the band
    assert len(fm.extend_chain([p], [], [])) == 0
    # the capacity protocol: offsets and alignments first, then DEBWT_ERANGE
    rng = np.random.default_rng(6)
    pats, chains = chains_for(R, mutated_reads(R, rng, 20), rng, 16)
    jobs, anchors = flatten(chains)
    ref = fm.extend_chain(pats, jobs, anchors)
    total = len(ref.cigars)
    assert total > len(jobs) // 2
    L = _lib.lib()
    buf, offs = api._patterns(pats)
    ja = (_lib.DebwtFmChainJob * len(jobs))()
    for k, (a, s, r, fa, n) in enumerate(jobs):
        ja[k].pattern, ja[k].strand, ja[k].record, ja[k].first_anchor, ja[k].n_anchors = a, s, r, fa, n
    aa = (_lib.DebwtFmAnchor * len(anchors))()
    for k, (q, dg) in enumerate(anchors):
        aa[k].qbeg, aa[k].diag = q, dg
    sc = _lib.DebwtFmScoring(1, 4, 6, 1)
    out = np.zeros(len(jobs), dtype=api._ALN_DTYPE)
    coff = np.zeros(len(jobs) + 1, dtype=np.uint64)
    cg = np.zeros(total, dtype=np.uint32)
    u32p, alnp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_lib.DebwtFmAln)

    def call(cap, cigar=True):
        return L.debwt_fm_extend_chain(fm._h, buf, api._p64(offs), len(pats), ja, len(jobs), aa, len(anchors), ctypes.byref(sc),
                                       16, out.ctypes.data_as(alnp), api._p64(coff), cg.ctypes.data_as(u32p) if cigar else None,
                                       cap)

    assert call(total - 1) == -5
    assert np.array_equal(coff, ref.offsets) and np.array_equal(out, ref.aln)
    assert call(total, cigar=False) == -5
    assert call(total) == 0 and np.array_equal(cg, ref.cigars)
    fm.close()


def check_chained_hits(R, pats, res, w, sc, min_score):
    """check_hits of test_fm_extend_gpu for map_chained: every mapped read is a valid alignment inside the band of its
    returned anchors, and its score is the reference DP of (read, strand, anchors, w)"""
    from debwt_amd import api as A
    mapped = 0
    for i, p in enumerate(pats):
        fl = int(res.flags[i])
        assert int(res.pattern[i]) == i
        if fl & A.MAP_UNMAPPED:
            assert int(res.score[i]) == 0 and len(res.ops(i)) == 0 and int(res.mapq[i]) == 0 and res.anchors(i) == []
            assert bool(fl & A.MAP_TOO_LONG) == (len(p) > 65535)
            continue
        mapped += 1
        strand, rec, an = fl & A.MAP_REVERSE, int(res.record[i]), res.anchors(i)
        score = int(res.score[i])
        assert len(an) >= 1 and int(res.diag[i]) == an[0][1]
        assert all(a[0] < b[0] and abs(a[1] - b[1]) <= w for a, b in zip(an, an[1:])) and an[-1][0] < len(p)
        assert score >= min_score and 0 <= int(res.sub[i]) <= score
        assert int(res.mapq[i]) == 60 * (score - int(res.sub[i])) // score
        assert int(res.tbeg[i]) == R.rs[rec] + int(res.offset[i])
        assert score == R.dp(p, strand, rec, an, w, sc)[0], (i, p)
        R.check(p, (i, strand, tuple(an), rec), w, sc, score, int(res.qbeg[i]), int(res.qend[i]), int(res.tbeg[i]),
                int(res.tend[i]), int(res.edits[i]), res.ops(i))
    return mapped


@pytest.mark.parametrize("name", ["pan_4x20k", "shared_ends_duplicates"])
def test_chained_mapper_exact_conditions(api, name):
    recs = golden_records(entry_named(name))
    R = ChainRef(recs)
    fm = index_with_text(api, recs)
    rng = np.random.default_rng(124)
    reads = mutated_reads(R, rng, 60, lo=30, hi=150)
    pats = [r[0] for r in reads] + ["N" * 40, "", "ACGT", "".join("ACGT"[int(x)] for x in rng.integers(0, 4, 80))]
    res = fm.map_chained(pats)
    st = fm.map_stats()
    assert st["reads"] == len(pats) and st["jobs"] == st["candidates"] and st["seeds"] >= st["candidates"]
    mapped = check_chained_hits(R, pats, res, 16, (1, 4, 6, 1), 30)
    assert mapped == st["mapped"] == int(res.mapped.sum())
    for i, (p, _, _, _, nedit) in enumerate(reads):                       # an unedited read of 30 bases or more is one MEM
        if nedit == 0:
            assert res.mapped[i] and int(res.score[i]) == len(p) and res.cigar(i) == f"{len(p)}M", i
    assert sum(1 for r in reads if r[4] == 0) >= 3
    assert not res.mapped[len(reads):len(reads) + 3].any()
    for kw in (dict(min_len=12, band=8, scoring=(2, 3, 0, 2), min_score=20, max_gap=40),
               dict(strands="forward", max_occ=2, max_cand=1)):
        r2 = fm.map_chained(pats, **kw)
        check_chained_hits(R, pats, r2, kw.get("band", 16), kw.get("scoring", (1, 4, 6, 1)), kw.get("min_score", 30))
        if kw.get("strands") == "forward":
            assert not (r2.flags & api.MAP_REVERSE).any()
    # map() itself is untouched by the new entry point
    plain = fm.map(pats)
    assert plain.anchors(0) is None and int(plain.mapped.sum()) >= 1
    fm.close()


DRIFT_SEED = 20241117


def test_chained_mapper_follows_drift(api):
    """40 reads of 1500..3000 bases from 4 random records of 20 kb, each with 4..8 indels of 10..40 bases of one sign (a
    drift of 100 diagonals or more), edits at least 60 bases apart: with band = 63 map_chained aligns every one of them
    over 90 % of its length at the planted locus; map, whose band stays on one diagonal, loses at least one."""
    rng = np.random.default_rng(DRIFT_SEED)
    recs = [rng.integers(0, 4, 20000).astype(np.uint8) for _ in range(4)]
    R = RefDP(recs)
    reads = drift_reads(R.strs, DRIFT_SEED + 1, 40)
    fm = index_with_text(api, recs)
    pats = [r[0] for r in reads]
    res = fm.map_chained(pats, band=63)
    for i, (p, strand, rec, a) in enumerate(reads):
        assert res.mapped[i], i
        assert (int(res.strand[i]), int(res.record[i])) == (strand, rec), i
        assert int(res.qend[i]) - int(res.qbeg[i]) >= 0.9 * len(p), (i, int(res.qbeg[i]), int(res.qend[i]), len(p))
        assert abs(int(res.tbeg[i]) - (R.rs[rec] + a)) <= 63, i
        assert len(res.anchors(i)) >= 2
    plain = fm.map(pats, band=63)
    short = [i for i, p in enumerate(pats) if int(plain.qend[i]) - int(plain.qbeg[i]) < 0.9 * len(p)]
    assert len(short) >= 1
    fm.close()
