"""The paired-end mapper (debwt_fm_map_pairs) on a collection without repeated 19-mers, where every statement about a
read can be derived from how it was cut: clean pairs against FMIndex.map of the same reads, mates without a seed against
the window alignment of the rescue (fm_path_ref.path_ref over the window of stage 3), a planted repeat that only the
partner resolves, the insert-size estimate, and the errors."""
import numpy as np
import pytest

from test_fm_extend_chain_gpu import ChainRef
from test_fm_extend_gpu import index_with_text
from test_fm_mems_gpu import revcomp
from test_fm_window_gpu import window_ref

pytestmark = pytest.mark.gpu
PROPER, RESCUED, REVERSE, UNMAPPED = 8, 16, 1, 2
K = 19
COPY = (400, 1900, 300)                                     # record 6: bases [1900, 2200) repeat [400, 700)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


@pytest.fixture(scope="module")
def world(api):
    rng = np.random.default_rng(20261018)
    recs = [rng.integers(0, 4, size=3000).astype(np.uint8) for _ in range(7)]
    a, b, n = COPY
    recs[6][b:b + n] = recs[6][a:a + n]
    R = ChainRef(recs)
    # no 19-mer occurs twice on either strand, the second copy set aside
    kmers = [s[i:i + K] for r, s in enumerate(R.strs) for i in range(len(s) - K + 1) if not (r == 6 and b <= i <= b + n - K)]
    both = set(kmers) | {revcomp(k) for k in kmers}
    assert len(set(kmers)) == len(kmers) and len(both) == 2 * len(kmers)
    fm = index_with_text(api, recs)
    yield R, fm, both
    fm.close()


def pair_at(R, rec, f, T, L=100):
    """the forward mate at offset f of record rec and the reverse mate that ends T bases after f"""
    s = R.strs[rec]
    return s[f:f + L], revcomp(s[f + T - L:f + T])


def clean_pairs(R, rng, count):
    r1, r2, truth = [], [], []
    for p in range(count):
        rec, T = p % 6, int(rng.integers(250, 351))
        f = int(rng.integers(0, 3000 - T + 1))
        fw, rv = pair_at(R, rec, f, T)
        swap = p % 2 == 1
        r1.append(rv if swap else fw)
        r2.append(fw if swap else rv)
        truth.append((rec, f, T, swap))
    return r1, r2, truth


def interleave(r1, r2):
    return [r for pr in zip(r1, r2) for r in pr]


def same_alignment(a, i, b, j):
    for name in ("record", "strand", "tbeg", "tend", "qbeg", "qend", "score", "edits", "offset"):
        assert int(getattr(a, name)[i]) == int(getattr(b, name)[j]), (name, i, j)
    assert a.cigar(i) == b.cigar(j)


def test_clean_pairs(api, world):
    R, fm, _ = world
    r1, r2, truth = clean_pairs(R, np.random.default_rng(1), 40)
    res = fm.map_pairs(r1, r2)
    st = fm.pair_stats()
    single = fm.map(interleave(r1, r2))
    assert len(res) == 80 and res.mapped.all() and single.mapped.all()
    assert ((res.flags & PROPER) != 0).all() and ((res.flags & RESCUED) == 0).all()
    for p, (rec, f, T, swap) in enumerate(truth):
        for x in (0, 1):
            same_alignment(res, 2 * p + x, single, 2 * p + x)
            assert int(res.diag[2 * p + x]) == int(single.diag[2 * p + x]) and int(res.mapq[2 * p + x]) == 60
        fw, rv = (2 * p + 1, 2 * p) if swap else (2 * p, 2 * p + 1)
        assert (int(res.record[fw]), int(res.strand[fw]), int(res.tbeg[fw]), int(res.cigar(fw) == "100M")) == (rec, 0, R.rs[rec] + f, 1)
        assert (int(res.record[rv]), int(res.strand[rv]), int(res.tend[rv])) == (rec, 1, R.rs[rec] + f + T)
        assert (int(res.pairs["tlen"][p]), int(res.pairs["pair_score"][p]), int(res.pairs["pair_sub"][p])) == (T, 200, 0)
    lo, hi = api.insert_bounds([t[2] for t in truth])
    assert (st["ins_lo"], st["ins_hi"], st["estimate_pairs"]) == (lo, hi, 40)
    assert (st["pairs"], st["proper"], st["rescued"]) == (40, 40, 0)


def seedless(R, both, rng, read):
    """the read with a substitution at every 16th base from a random phase: no exact stretch reaches 19 bases"""
    s = list(read)
    for j in range(int(rng.integers(0, 16)), len(s), 16):
        s[j] = "ACGT"[("ACGT".index(s[j]) + int(rng.integers(1, 4))) % 4]
    s = "".join(s)
    assert all(s[i:i + K] not in both for i in range(len(s) - K + 1))      # `both` holds both strands of the text
    return s


@pytest.fixture(scope="module")
def rescue_pairs(world):
    R, fm, both = world
    rng = np.random.default_rng(2)
    r1, r2, truth = clean_pairs(R, rng, 16)
    r2 = [seedless(R, both, rng, r) for r in r2]
    return r1, r2, truth


def test_rescue(world, rescue_pairs):
    R, fm, _ = world
    r1, r2, truth = rescue_pairs
    reads = interleave(r1, r2)
    single = fm.map(reads)
    assert all(single.mapped[0::2]) and not any(single.mapped[1::2])
    res = fm.map_pairs(r1, r2, insert=(200, 500))
    st = fm.pair_stats()
    assert (st["pairs"], st["proper"], st["rescue_jobs"], st["rescued"], st["ins_lo"], st["ins_hi"], st["estimate_pairs"]) == \
           (16, 16, 16, 16, 200, 500, 0)
    for p in range(16):
        a, b = 2 * p, 2 * p + 1
        same_alignment(res, a, single, a)
        assert int(res.flags[a]) & (PROPER | RESCUED | UNMAPPED) == PROPER
        assert int(res.flags[b]) & (PROPER | RESCUED | UNMAPPED) == PROPER | RESCUED
        # the window of stage 3 next to mate 1's alignment, mate 2 on the other strand
        strand, rec = int(res.strand[a]), int(res.record[a])
        job = (0, 1 - strand, rec) + ((int(res.tbeg[a]), int(res.tbeg[a]) + 500) if strand == 0 else
                                      (max(0, int(res.tend[a]) - 500), int(res.tend[a])))
        score, qbeg, qend, tbeg, tend, edits, ops = window_ref(R, r2[p], job, (1, 4, 6, 1))
        assert score >= 60                                   # 100 bases, 6 or 7 substitutions
        got = tuple(int(getattr(res, n)[b]) for n in ("record", "strand", "score", "qbeg", "qend", "tbeg", "tend", "edits"))
        assert got == (rec, 1 - strand, score, qbeg, qend, tbeg, tend, edits)
        assert [int(x) for x in res.ops(b)] == ops
        assert (int(res.diag[b]), int(res.offset[b]), int(res.sub[b]), int(res.mapq[b])) == (tbeg - qbeg, tbeg - R.rs[rec], 0, 60)
        fw, rv = (b, a) if strand else (a, b)
        assert int(res.pairs["tlen"][p]) == int(res.tend[rv]) - int(res.tbeg[fw])
        assert int(res.pairs["pair_score"][p]) == int(res.score[a]) + score
    off = fm.map_pairs(r1, r2, insert=(200, 500), max_rescue=0)
    assert fm.pair_stats()["rescue_jobs"] == 0 and fm.pair_stats()["proper"] == 0
    for p in range(16):
        same_alignment(off, 2 * p, single, 2 * p)
        assert int(off.flags[2 * p]) & (PROPER | RESCUED | UNMAPPED) == 0
        assert int(off.flags[2 * p + 1]) == UNMAPPED and int(off.score[2 * p + 1]) == 0 and off.cigar(2 * p + 1) == ""
        assert int(off.pairs["tlen"][p]) == 0


def test_repeat_resolved_by_the_partner(world):
    R, fm, _ = world
    a, b, n = COPY
    rng = np.random.default_rng(3)
    r1, r2, where = [], [], []
    for p in range(8):
        T = int(rng.integers(250, 351))
        if p % 2 == 0:                                      # mate 1 forward inside the second copy, mate 2 after it
            f = int(rng.integers(b + n + 100 - T, b + n - 100 + 1))
            m1, m2 = pair_at(R, 6, f, T)
            pos1 = f
        else:                                               # mate 1 reverse inside the second copy, mate 2 before it
            f = int(rng.integers(b + 100 - T, b - 100 + 1))
            m2, m1 = pair_at(R, 6, f, T)
            pos1 = f + T - 100
        assert b <= pos1 and pos1 + 100 <= b + n
        r1.append(m1)
        r2.append(m2)
        where.append((pos1, T))
    single = fm.map(interleave(r1, r2))
    res = fm.map_pairs(r1, r2, insert=(200, 500))
    for p, (pos1, T) in enumerate(where):
        i = 2 * p
        assert (int(single.mapq[i]), int(single.tbeg[i])) == (0, R.rs[6] + pos1 - (b - a))      # the first copy wins the tie
        assert (int(res.record[i]), int(res.tbeg[i]), int(res.tend[i])) == (6, R.rs[6] + pos1, R.rs[6] + pos1 + 100)
        assert int(res.flags[i]) & (PROPER | RESCUED | UNMAPPED) == PROPER and int(res.flags[i + 1]) & (PROPER | UNMAPPED) == PROPER
        assert (int(res.mapq[i]), int(res.mapq[i + 1]), int(res.sub[i])) == (60, 60, 100)
        assert int(res.pairs["tlen"][p]) == T


def test_bounds_and_flags(api, world):
    R, fm, _ = world
    r1, r2, _ = clean_pairs(R, np.random.default_rng(4), 10)
    with pytest.raises(api.DebwtError) as e:
        fm.map_pairs(r1, r2)
    assert e.value.code == -1 and "bounds" in str(e.value)
    assert fm.map_pairs(r1, r2, insert=(200, 500)).mapped.all()
    with pytest.raises(api.DebwtError) as e:
        fm.map_pairs(r1, r2, insert=(200, 500), strands="forward")
    assert e.value.code == -1
    for insert in ((500, 200), (0, 16385)):
        with pytest.raises(api.DebwtError) as e:
            fm.map_pairs(r1, r2, insert=insert)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        fm.map_pairs(r1, r2[:-1], insert=(200, 500))
    empty = fm.map_pairs([], [], insert=(200, 500))
    assert len(empty) == 0 and len(empty.pairs) == 0
