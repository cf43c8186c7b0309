"""Shared by the k-mer tests: the reference of debwt_fm_kmer_counts, debwt_fm_weak_trials and debwt_fm_correct written
literally from their definitions (a Counter over the records' k-mers), and the seeded read set the CPU, GPU and CLI tests
use."""
import functools
from collections import Counter

import numpy as np

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
SHORT, CLEAN, FIXED, WEAK = 1, 2, 4, 8
LEFT, RIGHT = 0, 1


def revcomp(w):
    return "".join(COMP.get(c, "N") for c in reversed(w.upper()))


def rand_dna(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def trials(counts, k, min_count):
    """(run_a, run_b, pos, window, kind) of the weak runs of one read's counts, runs ascending, left first"""
    nk, out, j = len(counts), [], 0
    while j < nk:
        if counts[j] >= min_count:
            j += 1
            continue
        a = j
        while j + 1 < nk and counts[j + 1] < min_count:
            j += 1
        b = j
        ln = b - a + 1
        if a > 0 and (ln >= k or b == nk - 1):
            out.append((a, b, a + k - 1, a, LEFT))
        if b < nk - 1 and (ln >= k or a == 0):
            out.append((a, b, b, b, RIGHT))
        j += 1
    return out


class Ref:
    """occ, cnt, profile and correct over the k-mers of the records (strings of ACGT)"""

    def __init__(self, strs, k, both):
        self.k, self.both = k, both
        self.c = Counter(s[j:j + k] for s in strs for j in range(len(s) - k + 1))

    def occ(self, w):
        w = w.upper()
        return self.c.get(w, 0) if all(ch in "ACGT" for ch in w) else 0

    def cnt(self, w):
        return min(self.occ(w) + (self.occ(revcomp(w)) if self.both else 0), 2 ** 32 - 1)

    def profile(self, p):
        return [self.cnt(p[j:j + self.k]) for j in range(len(p) - self.k + 1)]

    def correct(self, read, min_count, rounds):
        """(output read, flags, fixes, weak_before, weak_after, notes); notes: what happened, for the tests that assert
        the read set holds every case: ("fix", round, kind, pos), ("two", round) for a trial with two candidates"""
        k, r, notes = self.k, list(read), []
        if len(r) < k:
            return read, SHORT, 0, 0, 0, notes
        weak_before, fixes = None, 0
        for rnd in range(rounds):
            prof = self.profile("".join(r))
            weak = sum(1 for c in prof if c < min_count)
            if weak_before is None:
                weak_before = weak
            if not weak:
                break
            fix, done = [], set()
            for a, b, pos, window, kind in trials(prof, k, min_count):
                if a in done:
                    continue
                cand = []
                for x in "ACGT":
                    if x == r[pos].upper():
                        continue
                    w = r[window:window + k]
                    w[pos - window] = x
                    if self.cnt("".join(w)) >= min_count:
                        cand.append(x)
                if len(cand) == 2:
                    notes.append(("two", rnd))
                if len(cand) == 1:
                    fix.append((pos, cand[0]))
                    done.add(a)
                    notes.append(("fix", rnd, kind, pos))
            if not fix:
                break
            assert len({p for p, _ in fix}) == len(fix)           # the fixes of a round fall on distinct positions
            for pos, x in fix:
                r[pos] = x
            fixes += len(fix)
        out = "".join(r)
        weak_after = sum(1 for c in self.profile(out) if c < min_count)
        flags = CLEAN if weak_before == 0 else FIXED if weak_after == 0 else WEAK
        return out, flags, fixes, weak_before, weak_after, notes


@functools.lru_cache(maxsize=None)
def read_set(seed=20250117):
    """The seeded read set: 1,500 reads of 50-80 b from a random 3,000 b genome, each from either strand, with 1 %
    substitutions, plus 80 reads of a second haplotype of genome[1000:1200) that differs in one base (position 1100), and
    one record that holds a 16-mer equal to its own reverse complement.  Returns a dict: records (what is indexed, with
    the errors), truth (the same reads without them), genome, snp (the position and the two bases), palindrome."""
    rng = np.random.default_rng(seed)
    g = rand_dna(rng, 3000)
    truth, recs = [], []
    for _ in range(1500):
        m = int(rng.integers(50, 81))
        a = int(rng.integers(0, 3000 - m + 1))
        t = g[a:a + m]
        if rng.integers(0, 2):
            t = revcomp(t)
        e = list(t)
        for j in np.nonzero(rng.random(m) < 0.01)[0]:
            e[j] = "ACGT"[("ACGT".index(e[j]) + int(rng.integers(1, 4))) % 4]
        truth.append(t)
        recs.append("".join(e))
    alt = "ACGT"[("ACGT".index(g[1100]) + 1) % 4]
    h = g[:1100] + alt + g[1101:]
    for _ in range(80):
        m = int(rng.integers(50, 81))
        a = int(rng.integers(1101 - m, 1100 + 1))
        truth.append(h[a:a + m])
        recs.append(h[a:a + m])
    half = rand_dna(rng, 8)
    pal = half + revcomp(half)
    truth.append(rand_dna(rng, 30) + pal + rand_dna(rng, 30))
    recs.append(truth[-1])
    return {"records": recs, "truth": truth, "genome": g, "snp": (1100, g[1100], alt), "palindrome": pal}


def correction_queries(k, seed=7):
    """The records and, behind them, the reads made for one case each: shorter than k and empty (SHORT), an N in place
    of a base, a third base at the position where the two haplotypes differ (two candidates), a read of a foreign genome
    (one run over its whole length), lower case with one error, two errors closer than k, an error within k - 1 of
    each end."""
    S = read_set()
    g, (snp, _, _) = S["genome"], S["snp"]
    rng = np.random.default_rng(seed)

    def sub(s, j, to=None):
        x = to or "ACGT"[("ACGT".index(s[j].upper()) + 2) % 4]
        return s[:j] + x + s[j + 1:]

    third = [x for x in "ACGT" if x not in S["snp"][1:]][0]
    extra = [g[200:200 + k - 1], "",
             sub(g[300:370], 35, "N"),
             sub(g[snp - 30:snp + 40], 30, third),
             rand_dna(rng, 70),
             sub(g[400:470], 33).lower(),
             sub(sub(g[500:580], 30), 30 + k // 2),
             sub(g[600:670], 3), sub(g[700:770], 66),
             g[800:870].lower()]
    return S["records"] + extra


def kmer_queries(k, seed=11):
    """The records and extra patterns: empty, of length k - 1, k and k + 1, lower case, an N first, last and in the middle,
    k-mers that are their own reverse complement (even k), a read of a foreign genome"""
    S = read_set()
    rng = np.random.default_rng(seed)
    r = [s for s in S["records"] if len(s) >= 66][:4]
    half = r[0][:k // 2]
    extra = ["", r[0][:k - 1] if k > 1 else "", r[1][:k], r[2][:k + 1], r[3].lower(), "N" + r[0][1:], r[1][:-1] + "N",
             r[2][:33] + "N" + r[2][34:], half + revcomp(half), "AC" + S["palindrome"] + "GT", "ACGTACGTTGCATGCAACGT",
             rand_dna(rng, 75)]
    return S["records"] + extra


@functools.lru_cache(maxsize=None)
def ref_of(k, both):
    return Ref(read_set()["records"], k, both)


@functools.lru_cache(maxsize=None)
def corrected(k, min_count, both, rounds):
    """the reference's correction of correction_queries(k): a list of (out, flags, fixes, weak_before, weak_after, notes)"""
    R = ref_of(k, both)
    return [R.correct(p, min_count, rounds) for p in correction_queries(k)]
