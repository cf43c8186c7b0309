"""The assertions of tests/test_fm_geometry_gpu.py run on the CPU against a stand-in index that answers from the
definition: with the right answers every test passes, and with one answer made wrong on purpose -- two rows of the suffix
array swapped, an interval one row too long, a substring shifted by one base, a padding bit, a k-mer count, two overlap
hits out of record order, a search interval, the interval of a reverse-strand MEM -- the test that looks at it fails.  No
GPU and no library call: this shows that the GPU tests can fail, and where."""
import types

import numpy as np
import pytest

import fm_definition as F
import test_fm_geometry_gpu as T
from debwt_amd import api as A

CASES = ("n385", "short_1to3_x500")


class StandIn:
    """what the GPU tests use of FMIndex, answered by a Definition; `wrong` names the one answer that is falsified"""

    def __init__(self, D, s, wrong):
        self.D, self.s, self.wrong, self.sa, self.last = D, s, wrong, D.sa.copy(), {}
        if wrong == "sa_swap":
            lo, hi = max((D.interval(c) for c in "ACGT"), key=lambda r: r[1] - r[0])
            self.sa[[lo, lo + 1]] = self.sa[[lo + 1, lo]]

    def info(self):
        return {"n": self.D.n, "nrec": self.D.nrec, "sa_sample": self.s, "samples": (self.D.n + self.s - 1) // self.s,
                "census": self.D.census()}

    def record_starts(self):
        return self.D.starts.copy()

    def samples(self):
        return self.sa[::self.s].astype(np.uint64)

    def ranges(self, pats):
        r = np.array([self.D.interval(p) for p in pats], dtype=np.uint64).reshape(-1, 2)
        if self.wrong == "interval_off_by_one":
            r[r[:, 1] > r[:, 0], 1] += 1
        return r

    def count(self, pats):
        r = self.ranges(pats)
        return r[:, 1] - r[:, 0]

    def locate(self, pats, max_per_pattern=None):
        rows = [self.sa[slice(*self.D.interval(p))] for p in pats]
        return [(g if max_per_pattern is None else g[:max_per_pattern]).astype(np.uint64) for g in rows]

    def extract(self, jobs):
        shift = 1 if self.wrong == "extract_shift" else 0
        return [(self.D.substring(j[0]) if len(j) == 1 else
                 self.D.substring(j[0], max(j[1] - (shift if j[1] % 32 == 0 else 0), 0), j[2])).encode() for j in jobs]

    def restore_text(self):
        pass

    def extract_stats(self):
        return {"jobs": 0, "bases": self.D.n, "steps": self.D.n - 1}

    def text(self):
        w, sp = F.packed_text(self.D.records)
        if self.wrong == "text_pad":
            w[(self.D.n + 31) >> 5] ^= np.uint64(3)             # one code of the packed text
        return w, sp

    def _offsets(self, lists):
        offs = np.zeros(len(lists) + 1, dtype=np.uint64)
        np.cumsum([len(x) for x in lists], out=offs[1:])
        return offs, [h for x in lists for h in x]

    def kmer_counts(self, reads, k, strands="forward"):
        prof = [self.D.kmer_profile(p, k, strands == "both") for p in reads]
        if self.wrong == "kmer" and k == 12:
            prof = [[c + (1 if j == len(x) - 1 else 0) for j, c in enumerate(x)] for x in prof]
        self.last["q"] = 12 if k >= 12 else 0
        offs, flat = self._offsets(prof)
        return A.KmerResult(offs, np.array(flat, dtype=np.uint32))

    def kmer_stats(self):
        return {"table_q": self.last["q"]}

    def _overlap_result(self, lists):
        offs, flat = self._offsets(lists)
        self.last["runs"] = len(flat)
        return A.OverlapResult(self, offs, np.array(flat, dtype=A._OVERLAP_DTYPE))

    def overlaps(self, qs, min_overlap=20, strands="forward", longest=False):
        lists = [self.D.overlaps(q, min_overlap, strands == "both", longest) for q in qs]
        if self.wrong == "overlap_record_order":
            lists = [[x[1], x[0]] + x[2:] if len(x) > 1 else x for x in lists]
        return self._overlap_result(lists)

    def overlaps_stats(self):
        return {"runs": self.last["runs"]}

    def overlaps_mm(self, qs, min_overlap=20, mismatches=1, error_permille=0, strands="forward", longest=False):
        if any(len(q) > 1024 for q in qs):
            raise A.DebwtError(-1)
        return self._overlap_result([self.D.overlaps_mm(q, min_overlap, mismatches, strands == "both", longest) for q in qs])

    def search(self, pats, mismatches=1, strands="forward", best=False):
        lists = [self.D.search(p.decode(), mismatches, strands == "both", best) for p in pats]
        if self.wrong == "search_interval":
            lists = [[(a, b + (1 if m else 0), m, t) for a, b, m, t in x] for x in lists]
        offs, flat = self._offsets(lists)
        return A.SearchResult(self, offs, np.array([h[:2] for h in flat], dtype=np.uint64).reshape(-1, 2),
                              np.array([h[2] for h in flat], dtype=np.uint8), np.array([h[3] for h in flat], dtype=np.uint8))

    def mems(self, reads, min_len=19, strands="forward"):
        lists = [self.D.mems(p, min_len, strands == "both") for p in reads]
        offs, flat = self._offsets(lists)
        ranges = []
        for p, x in zip(reads, lists):
            for t, a, b in x:
                w = p[a:b].upper()
                ranges.append(self.D.interval(w if t == 0 or self.wrong == "mem_strand" else F.revcomp(w)))
        return A.MemResult(self, offs, np.array([h[1:] for h in flat], dtype=np.uint32).reshape(-1, 2),
                           np.array(ranges, dtype=np.uint64).reshape(-1, 2), np.array([h[0] for h in flat], dtype=np.uint8))

    def close(self):
        pass


def stand_in_api(wrong=None):
    def open_(words, n, hash_rows, dollar_row, samples, sa_sample=32):
        D = next(F.definition_of(c) for c in CASES if F.definition_of(c).words is words)
        assert n == D.n and dollar_row == D.dollar_row and np.array_equal(samples, D.sa[::sa_sample].astype(np.uint64))
        return StandIn(D, sa_sample, wrong)
    return types.SimpleNamespace(FMIndex=types.SimpleNamespace(open=open_), DebwtError=A.DebwtError)


def run(test, api, name, s):
    return test(api, name) if test is T.test_kmer_counts else test(api, name, s)


ALL = (T.test_index_facts, T.test_ranges, T.test_locate, T.test_extract_and_restore, T.test_kmer_counts, T.test_overlaps,
       T.test_search, T.test_mems)


@pytest.mark.parametrize("name", CASES)
def test_right_answers_pass(name):
    for test in ALL:
        run(test, stand_in_api(), name, 32)


@pytest.mark.parametrize("wrong,test,name,s", [
    ("sa_swap", T.test_locate, "n385", 1024),                   # a sorted comparison would let this through
    ("sa_swap", T.test_locate, "short_1to3_x500", 1),
    ("sa_swap", T.test_index_facts, "n385", 1),
    ("interval_off_by_one", T.test_ranges, "n385", 1),
    ("interval_off_by_one", T.test_ranges, "short_1to3_x500", 1),
    ("extract_shift", T.test_extract_and_restore, "n385", 1),
    ("text_pad", T.test_extract_and_restore, "short_1to3_x500", 1),
    ("kmer", T.test_kmer_counts, "n385", 32),
    ("overlap_record_order", T.test_overlaps, "short_1to3_x500", 1),
    ("search_interval", T.test_search, "n385", 1),
    ("mem_strand", T.test_mems, "short_1to3_x500", 1),
], ids=lambda v: v.__name__ if callable(v) else str(v))
def test_a_wrong_answer_fails(wrong, test, name, s):
    run(test, stand_in_api(), name, s)                           # the same test passes with the right answers
    with pytest.raises(AssertionError):
        run(test, stand_in_api(wrong), name, s)
