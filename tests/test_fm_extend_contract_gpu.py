"""The two seed-extension kernels against the ONE alignment that include/debwt_hip.h documents (fm_path_ref.path_ref):
every field of the result and the whole CIGAR, exactly.  (a) tie-rich collections, every band width at which the launch
code or the kernels take another path, scorings up to the limit of 255; (b) a chain whose text window does not fit the
LDS budget, so that k_fm_extend_chain reads the text from memory; (c) small bands in a lane group that one long job of the
batch has widened.  What each part relies on is asserted from the test's own arithmetic, not from a statistic."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden_records
from fm_chain_ref import centres, chain_dp_rows
from fm_path_ref import path_ref
from test_fm_extend_chain_gpu import ChainRef, chains_for, flatten, random_chain
from test_fm_extend_gpu import index_with_text, jobs_for, mutated_reads
from test_fm_search_gpu import entry_named

pytestmark = pytest.mark.gpu
SCORINGS = [(1, 4, 6, 1), (2, 3, 0, 2), (1, 1, 0, 1), (255, 255, 0, 1), (255, 255, 255, 255), (1, 255, 255, 255),
            (255, 1, 0, 1), (3, 2, 1, 1)]
BANDS = [0, 1, 7, 15, 16, 31, 32, 63]
KERNELS = ["extend", "extend_chain"]
COLLECTIONS = ["homopolymers_tandem", "shared_ends_duplicates"]
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
LDS_BUDGET = 64 << 10                                       # FM_EXT_LDS_BUDGET of debwt_hip.hip, see test_the_launch_code_is_the_one_modelled_here


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


@pytest.fixture(scope="module")
def world(api):
    """(ChainRef, index with text) of a collection, built once for the module"""
    made = {}

    def get(name, recs=None):
        if name not in made:
            recs = golden_records(entry_named(name)) if recs is None else recs
            made[name] = (ChainRef(recs), index_with_text(api, recs))
        return made[name]

    yield get
    for _, fm in made.values():
        fm.close()


def run(fm, kernel, pats, chains, sc, w, cigar=True):
    """chains: (pattern, strand, record, anchors); for `extend` every chain has one anchor and goes as a fixed-band job"""
    if kernel == "extend":
        assert all(len(an) == 1 for _, _, _, an in chains)
        return fm.extend(pats, [(k, s, an[0][1], r) for k, s, r, an in chains], scoring=sc, band=w, cigar=cigar)
    jobs, anchors = flatten(chains)
    return fm.extend_chain(pats, jobs, anchors, scoring=sc, band=w, cigar=cigar)


def reference(R, pats, chain, w, sc, info=None):
    k, strand, rec, an = chain
    return path_ref(R.query(pats[k], strand), R.text, R.rs[rec], R.re[rec], an, w, sc, info)


def result(res, j):
    return (int(res.score[j]), int(res.qbeg[j]), int(res.qend[j]), int(res.tbeg[j]), int(res.tend[j]), int(res.edits[j]),
            [int(x) for x in res.ops(j)])


def test_the_launch_code_is_the_one_modelled_here():
    """parts (b) and (c) derive the branch and the launch shapes they reach from the budget constant, the group widths and
    the widening loop of the host code, which native_group and launch_shape below repeat: if one of those lines changes,
    the tests no longer cover what they say, so this fails instead"""
    src = open(os.path.join(ROOT, "debwt_amd", "csrc", "debwt_hip.hip")).read()
    m = re.search(r"constexpr u32 FM_EXT_LDS_BUDGET = (\d+)u << (\d+);", src)
    assert m and int(m.group(1)) << int(m.group(2)) == LDS_BUDGET
    assert src.count("const int G = w < 16 ? 16 : w < 32 ? 32 : 64;") == 1                        # fm_extend_run
    assert src.count("const int G = 2 * w + 1 <= 16 ? 16 : 2 * w + 1 <= 32 ? 32 : 64;") == 1      # fm_chain_run
    widen = ("        int g = G;\n        u32 block = 256;\n"
             "        if ((u64)(block / g) * lds_job > FM_EXT_LDS_BUDGET) block = 64;\n"
             "        while ((u64)(block / g) * lds_job > FM_EXT_LDS_BUDGET && g < 64) g *= 2;\n")
    assert src.count(widen) == 2                                                                # both launchers
    assert src.count("lds_job = std::max<u32>(lds_job, (u32)(((m + 1) / 2 + (m + 2 * w + 3) / 4 + 3) & ~3ull));") == 1
    assert src.count("if ((m + 1) / 2 + ((u64)d.wn + 3) / 4 + 3 > FM_EXT_LDS_BUDGET) d.wn = 0;") == 1
    assert src.count("lds_job = std::max<u32>(lds_job, (u32)(((m + 1) / 2 + ((u64)d.wn + 3) / 4 + 3) & ~3ull));") == 1


# ---- (a) the exact alignment ------------------------------------------------------------------------------------------
# The scorings rotate over the bands; the offset of a (kernel, collection) is chosen so that bands 32 and 63 never meet
# (1,255,255,255): there a gap costs 510 and a read of 90 bases scores 90 at most, so no path holds a gap and none steps
# from band index 63 to 64.  (255,255,255,255), whose gaps cost two matches, is run at w = 32 and w = 63 in two more cases
# of every (kernel, collection), so that the two band indices of a lane, the prefix scan's k * e offset up to 126 x 255
# and the bit that crosses from lane 63 to lane 0 meet the largest penalties.
OFFSET = {("extend", 0): 0, ("extend", 1): 2, ("extend_chain", 0): 4, ("extend_chain", 1): 1}
CASES = [(w, None) for w in BANDS] + [(32, SCORINGS[4]), (63, SCORINGS[4])]
CASE_IDS = [f"w{w}" if sc is None else f"w{w}-all255" for w, sc in CASES]
# seeds chosen on the CPU with the reference alone (the conditions are asserted again below): the smallest seed whose
# jobs hold a tie on a returned path and, for w >= 32, a path that steps from band index 63 to 64
SEEDS = {("extend", 1, 6): 6, ("extend", 1, 7): 9, ("extend_chain", 0, 6): 2, ("extend_chain", 1, 7): 11,
         ("extend", 0, 8): 5, ("extend", 0, 9): 6, ("extend", 1, 8): 6, ("extend", 1, 9): 21,
         ("extend_chain", 0, 8): 2, ("extend_chain", 0, 9): 1, ("extend_chain", 1, 8): 2, ("extend_chain", 1, 9): 11}


def make_case(R, kernel, ci, n):
    """the jobs of one (kernel, collection, case): (pats, chains, w, scoring, references, what the references met)"""
    w, sc = CASES[n]
    if sc is None:
        sc = SCORINGS[(n + OFFSET[kernel, ci]) % 8]
    pats, chains = build_jobs(R, kernel, w, SEEDS.get((kernel, ci, n), 0))
    infos = [{} for _ in chains]
    refs = [reference(R, pats, c, w, sc, info) for c, info in zip(chains, infos)]
    return pats, chains, w, sc, refs, infos


@pytest.fixture(scope="module")
def contract(world):
    """every case of part (a) with its references, computed once and left unchanged"""
    return {(kernel, ci, n): make_case(world(COLLECTIONS[ci])[0], kernel, ci, n)
            for kernel in KERNELS for ci in range(len(COLLECTIONS)) for n in range(len(CASES))}


def build_jobs(R, kernel, w, seed):
    rng = np.random.default_rng(seed)
    reads = mutated_reads(R, rng, 12, hi=90)
    if kernel == "extend":
        pats, jobs = jobs_for(R, reads, rng, w)
        return pats, [(k, s, r, [(0, d)]) for k, s, d, r in jobs]
    return chains_for(R, reads, rng, w)


def gaps_possible(sc, m=90):
    """can a path of a read of m bases hold a gap at all?  a gap costs o + e at least and the score before it is below m a"""
    return sc[2] + sc[3] < m * sc[0]


@pytest.mark.parametrize("n", range(len(CASES)), ids=CASE_IDS)
@pytest.mark.parametrize("ci", range(len(COLLECTIONS)), ids=COLLECTIONS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_exact_alignment(world, contract, kernel, ci, n):
    R, fm = world(COLLECTIONS[ci])
    pats, chains, w, sc, refs, infos = contract[kernel, ci, n]
    assert len(chains) >= 30 and sum(r[0] > 0 for r in refs) >= 12
    if w == 0:
        # one diagonal: E and F are -inf in every cell, so no cell has two sources; what the rule decides is the end cell
        assert any(i["end_ties"] for i in infos)
    elif gaps_possible(sc):
        assert sum(i["ties"] for i in infos) > 0
    if w >= 32:
        assert sum(i["cross64"] for i in infos) > 0
    res = run(fm, kernel, pats, chains, sc, w)
    assert len(res) == len(chains)
    for j, want in enumerate(refs):
        assert result(res, j) == want, (chains[j], pats[chains[j][0]], w, sc)
    assert int(res.offsets[-1]) == len(res.cigars) == sum(len(r[6]) for r in refs)
    so = run(fm, kernel, pats, chains, sc, w, cigar=False)
    for j, want in enumerate(refs):
        assert (int(so.score[j]), int(so.qend[j]), int(so.tend[j])) == (want[0], want[2], want[4])


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_band_meets_a_tie(contract, kernel):
    """over the collections, every band of every kernel has a returned path on which the tie rule decided (w = 0: among
    end cells), whatever scorings the rotation gave it"""
    for n, w in enumerate(BANDS):
        infos = [i for ci in range(len(COLLECTIONS)) for i in contract[kernel, ci, n][5]]
        assert sum(i["end_ties"] if w == 0 else i["ties"] for i in infos) > 0, (kernel, w)


# ---- (b) a text window beyond the LDS budget: the text is read from memory (J.wn == 0) -----------------------------------
ZONE_W, SEG, ZONE, NSEG = 63, 100, 140, 30


def drifting_chain(R, rec, first, step, rng):
    """30 segments of 100 query rows copied from the text; between two segments 140 random query bases in which every row
    is an anchor stepping `step` diagonals.  first: the first diagonal's offset into the record."""
    parts, an, d = [], [(0, R.rs[rec] + first)], R.rs[rec] + first
    for x in range(NSEG):
        q = x * (SEG + ZONE)
        parts.append(R.text[q + d:q + d + SEG])
        if x + 1 < NSEG:
            parts.append("".join("ACGT"[int(c)] for c in rng.integers(0, 4, ZONE)))
            for z in range(ZONE):
                d += step
                an.append((q + SEG + z, d))
    return "".join(parts), an


@pytest.fixture(scope="module")
def long_record(world):
    rng = np.random.default_rng(300000)
    recs = [rng.integers(0, 4, 500).astype(np.uint8), rng.integers(0, 4, 300000).astype(np.uint8)]
    R, fm = world("two_records_300k", recs)
    return R, fm, [CODE.get(c, 5) for c in R.text]


@pytest.mark.parametrize("step", [63, -63], ids=["up", "down"])
def test_text_read_from_memory(long_record, step):
    R, fm, tcodes = long_record
    assert R.rs[1] != 0
    w, sc = ZONE_W, (100, 1, 0, 1)
    m = NSEG * SEG + (NSEG - 1) * ZONE
    first = 1000 if step > 0 else len(R.strs[1]) - 1000 - m
    p, an = drifting_chain(R, 1, first, step, np.random.default_rng(7060 + step))
    assert (len(p), len(an)) == (m, (NSEG - 1) * ZONE + 1) == (7060, 4061)
    # the window the launch code would stage: the columns of all allowed cells, clipped to the record.  With the query
    # beside it, it exceeds FM_EXT_LDS_BUDGET (pinned by test_the_launch_code_is_the_one_modelled_here), so it is not staged: wn = 0.
    cen = centres(an, m)
    lo = max(R.rs[1], min(i + c - w for i, c in enumerate(cen)))
    hi = min(R.re[1] - 1, max(i + c + w for i, c in enumerate(cen)))
    window = hi - lo + 1
    assert step < 0 or window == 262966
    assert (m + 1) // 2 + (window + 3) // 4 + 3 > LDS_BUDGET
    if step < 0:
        assert min(i + c - w for i, c in enumerate(cen)) < an[0][1] - w - 240000      # far below column 0 of the job
    chains = [(0, 0, 1, an)]
    want = chain_dp_rows([CODE[c] for c in p], tcodes, R.rs[1], R.re[1], an, w, sc)
    ref = path_ref(p, R.text, R.rs[1], R.re[1], an, w, sc)
    assert ref[0] == want
    res = run(fm, "extend_chain", [p], chains, sc, w)
    print("score", int(res.score[0]), "reference", want, "query span", int(res.qend[0]) - int(res.qbeg[0]))
    assert int(res.score[0]) == want
    assert result(res, 0) == ref
    if step > 0:
        # a segment scores 10 000 and a zone costs at most 140 x (1 + 63) when every row pays a mismatch and 63 deleted
        # bases: the path through all segments is among the candidates, and nothing shorter comes near it
        assert want >= NSEG * SEG * 100 - (NSEG - 1) * ZONE * 64
        assert int(res.qend[0]) - int(res.qbeg[0]) >= 0.9 * m
    else:
        # The mirrored job cannot be asked for 0.9 m: along a path text positions never decrease, and from one segment to
        # the next the diagonal falls by 8 820 while the query advances by 240, so no path joins two segments.  The best
        # one stays inside a segment (100 matches, plus what chance adds at its ends).  What this case adds is the text
        # read from memory at columns far below column 0 of the job, with a result that is still exact.
        assert SEG * 100 <= want < 2 * SEG * 100
        assert int(res.qend[0]) - int(res.qbeg[0]) < 2 * SEG
    so = run(fm, "extend_chain", [p], chains, sc, w, cigar=False)
    assert (int(so.score[0]), int(so.qend[0]), int(so.tend[0])) == (want, ref[2], ref[4])


# ---- (c) small bands in a widened lane group ----------------------------------------------------------------------------
LONG_M = [6000, 24000, 46000, 60000]
# (block, lanes per job) that the launch code derives for a batch whose largest job has LONG_M[x] bases; the native
# group of the band is 16 lanes except for the chain kernel at w = 15 (31 band indices: 32 lanes)
SHAPES = {"extend": [(64, 16), (64, 32), (64, 64), (64, 64)],
          "extend_chain": [(64, 16), (64, 32), (64, 32), (64, 64)],
          ("extend_chain", 15): [(256, 32), (64, 32), (64, 32), (64, 64)]}


def native_group(kernel, w):
    if kernel == "extend":
        return 16 if w < 16 else 32 if w < 32 else 64
    return 16 if 2 * w + 1 <= 16 else 32 if 2 * w + 1 <= 32 else 64


def launch_shape(kernel, w, lds_job):
    """(block, lanes per job) as the launch code derives them from the largest staged job of a batch"""
    g, block = native_group(kernel, w), 256
    if block // g * lds_job > LDS_BUDGET:
        block = 64
    while block // g * lds_job > LDS_BUDGET and g < 64:
        g *= 2
    return block, g


def staged_bytes(kernel, m, w, reclen):
    """LDS of one job whose diagonal is its record's first base: the query, 4 bits a base, and the text window, 2 bits a
    base.  A fixed band stages all its m + 2w columns, about 0.75 m in all.  A chain stages the columns of its allowed
    cells clipped to the record: text positions rs .. min(re - 1, rs + m - 1 + w)."""
    window = m + 2 * w if kernel == "extend" else min(reclen, m + w)
    return ((m + 1) // 2 + (window + 3) // 4 + 3) & ~3


@pytest.fixture(scope="module")
def long_pattern(world):
    """the whole of record 0 with a 3-base deletion and a 3-base insertion, then random bases up to the length limit; a
    job of length m takes its first m bases"""
    R, _ = world("pan_4x20k")
    rng = np.random.default_rng(46000)
    s = R.strs[0]
    ins = "".join("ACGT"[(CODE[s[4000 + x]] + 1 + x) % 4] for x in range(3))       # none equals the base it displaces
    full = s[:2000] + s[2003:4000] + ins + s[4000:]
    full += "".join("ACGT"[int(c)] for c in rng.integers(0, 4, 65535 - len(full)))
    return full, [CODE.get(c, 5) for c in R.text]


@pytest.fixture(scope="module")
def long_scores(world, long_pattern):
    """the reference score of the long job for every (w, m), computed once and left unchanged.  Query row i has an allowed
    cell only while i + rs - w < re, so rows from the record's length + w on add nothing: the DP runs on the rows before."""
    R, _ = world("pan_4x20k")
    full, tcodes = long_pattern
    out, done = {}, {}
    for w in (0, 7, 15):
        for m in LONG_M:
            rows = min(m, len(R.strs[0]) + w)
            if (w, rows) not in done:
                done[w, rows] = chain_dp_rows([CODE[c] for c in full[:rows]], tcodes, R.rs[0], R.re[0], [(0, R.rs[0])], w,
                                              (1, 4, 6, 1))
            out[w, m] = done[w, rows]
    return out


@pytest.mark.parametrize("w", [0, 7, 15])
@pytest.mark.parametrize("kernel", KERNELS)
def test_small_band_in_a_widened_group(world, long_pattern, long_scores, monkeypatch, kernel, w):
    R, fm = world("pan_4x20k")
    full, _ = long_pattern
    sc = (1, 4, 6, 1)
    monkeypatch.delenv("DEBWT_FM_EXTEND_BYTES", raising=False)
    # 6 000, 24 000 and 46 000 lie one in each step of debwt_fm_extend's launch code (block = 64, g = 32, g = 64 at about
    # 0.75 m against 64 KiB).  A chain stages its window clipped to the record of 20 000 bases, so its last step needs
    # m / 2 + 5 000 > 32 KiB: 60 000 is run as well, for both kernels.
    shapes = [launch_shape(kernel, w, staged_bytes(kernel, m, w, len(R.strs[0]))) for m in LONG_M]
    assert shapes == SHAPES.get((kernel, w), SHAPES[kernel]), shapes
    if kernel == "extend":
        assert len(set(shapes[:3])) == 3
    assert {(64, g) for g in (16, 32, 64) if g >= native_group(kernel, w)} <= set(shapes), shapes
    rng = np.random.default_rng(100 * w + len(kernel))
    reads = mutated_reads(R, rng, 30)
    pats = [r[0] for r in reads]
    short = []
    for k, (p, strand, rec, diag, _) in enumerate(reads):
        d0 = diag + int(rng.integers(-(w + 3), w + 4))
        short.append((k, strand, rec, [(0, d0)] if kernel == "extend" else random_chain(rng, len(p), d0, w)))
    refs = [reference(R, pats, c, w, sc) for c in short]
    assert sum(r[0] > 0 for r in refs) >= 20
    alone = run(fm, kernel, pats, short, sc, w)
    for j, want in enumerate(refs):
        assert result(alone, j) == want, (short[j], w)
    # the short jobs alone leave the group as narrow as the band allows
    assert launch_shape(kernel, w, max(staged_bytes(kernel, len(p), w, 20000) for p in pats)) == (256, native_group(kernel, w))
    at = len(short) // 2
    for m in LONG_M:
        long = (len(pats), 0, 0, [(0, R.rs[0])])
        mixed = short[:at] + [long] + short[at:]
        res = run(fm, kernel, pats + [full[:m]], mixed, sc, w)
        assert fm.extend_stats()["batches"] == 1 and fm.extend_stats()["jobs"] == len(mixed)
        keep = [j for j in range(len(mixed)) if j != at]
        assert np.array_equal(res.aln[keep], alone.aln)
        got_ops = [x for j in keep for x in res.ops(j)]
        assert np.array_equal(np.asarray(got_ops, dtype=np.uint32), alone.cigars)
        assert [int(res.offsets[j + 1]) - int(res.offsets[j]) for j in keep] == [len(alone.ops(j)) for j in range(len(short))]
        for j, want in zip(keep, refs):
            assert result(res, j) == want, (mixed[j], w, m)
        assert int(res.score[at]) == long_scores[w, m], (w, m)
        ops = [int(x) for x in res.ops(at)]
        if w >= 7:
            assert (3 << 4 | 2) in ops and (3 << 4 | 1) in ops, (w, m)
            assert int(res.qend[at]) - int(res.qbeg[at]) >= min(m, 20000) - 2 * w
        one = run(fm, "extend", [full[:m]], [(0, 0, 0, long[3])], sc, w)
        two = run(fm, "extend_chain", [full[:m]], [(0, 0, 0, long[3])], sc, w)
        for other in (one, two):
            assert other.aln[0] == res.aln[at] and [int(x) for x in other.ops(0)] == ops, (w, m)
