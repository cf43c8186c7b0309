"""Shared by the tests of overlaps with mismatches: the reference of debwt_fm_overlaps_mm straight from its definition
(every record against every length, column by column) and the mutated read set the GPU and CLI tests query."""
import numpy as np

from overlap_ref import CONTAINS, WHOLE, extra_queries, synthetic_reads

_LUT = np.full(256, 255, dtype=np.uint8)                 # a query character outside ACGTacgt: a code that equals nothing
for _i, _c in enumerate("ACGT"):
    _LUT[ord(_c)] = _LUT[ord(_c.lower())] = _i
_PAD = 254                                               # past a record's end: equals nothing either
_cache = {}


def _matrix(strs):
    """(records as a padded uint8 matrix, one record per column so that the first L bases of all are contiguous; their
    lengths), made once per list"""
    hit = _cache.get(id(strs))
    if hit is None or hit[0] is not strs:
        lens = np.array([len(s) for s in strs], dtype=np.int64)
        R = np.full((int(lens.max()), len(strs)), _PAD, dtype=np.uint8)
        for j, s in enumerate(strs):
            R[:len(s), j] = _LUT[np.frombuffer(s.encode(), dtype=np.uint8)]
        hit = _cache[id(strs)] = (strs, R, lens)
    return hit[1], hit[2]


def brute(strs, q, min_overlap, K, permille=0, strand=0):
    """(record, length, strand, CONTAINS | WHOLE | mm << 8) of the query string q as given (the caller passes the reverse
    complement for strand 1), by (length descending, record ascending): for every L the mismatching columns of every
    record's first L bases against q's last L characters, counted."""
    R, lens = _matrix(strs)
    qc = _LUT[np.frombuffer(q.encode(), dtype=np.uint8)]
    m, out = len(q), []
    for L in range(min(m, R.shape[0]), min_overlap - 1, -1):
        mm = np.count_nonzero(R[:L] != qc[m - L:, None], axis=0)
        ok = (lens >= L) & (mm <= K)
        if permille:
            ok &= 1000 * mm <= permille * L
        for j in np.nonzero(ok)[0].tolist():
            out.append((j, L, strand, (CONTAINS if L == lens[j] else 0) | (WHOLE if L == m else 0) | (int(mm[j]) << 8)))
    return out


def mutated_reads(seed=7):
    """(reads, originals): overlap_ref.synthetic_reads() with substitutions planted per read.  Read i gets i % 3 at random
    positions; instead of them every 17th read gets one at position 0, every 19th one at its last position and every 23rd
    two at positions 30 and 31 (the later rule wins).  A substitution always changes the base."""
    orig = synthetic_reads()
    rng = np.random.default_rng(seed)
    out = []
    for i, s in enumerate(orig):
        pos = sorted(int(x) for x in rng.choice(len(s), size=i % 3, replace=False))
        if i % 17 == 0:
            pos = [0]
        if i % 19 == 0:
            pos = [len(s) - 1]
        if i % 23 == 0:
            pos = [30, 31]
        t = list(s)
        for p in pos:
            t[p] = "ACGT"[("ACGT".index(t[p]) + 1 + int(rng.integers(0, 3))) % 4]
        out.append("".join(t))
    return out, orig


def queries(strs, orig, min_overlap=20):
    """every 4th mutated read, every 9th original (unmutated) read, the edge queries of overlap_ref"""
    return strs[::4] + orig[1::9] + extra_queries(strs, min_overlap)
