"""Shared by the overlap tests: the reference of debwt_fm_overlaps straight from its definition, and the synthetic read
set the GPU and CLI tests query."""
import numpy as np

COMP = str.maketrans("ACGTacgt", "TGCAtgca")
CONTAINS, WHOLE = 1, 2


def revcomp(p):
    return "".join(c.translate(COMP) if c in "ACGTacgt" else "N" for c in reversed(p))


class Ref:
    """A dictionary from every record prefix of length >= min_overlap to the records that start with it (ascending),
    looked up for every suffix of the query: the definition, literally.  On a collection whose prefixes would not fit
    (more than 2 * 10^7 characters of them) the dictionary holds the prefixes of length min_overlap only and every
    candidate is compared in full: the same set, by the same comparison of strings."""

    def __init__(self, strs, min_overlap):
        self.strs, self.min_overlap = strs, min_overlap
        self.longest = max(len(s) for s in strs)
        self.full = sum(len(s) * (len(s) + 1) // 2 for s in strs) <= 20_000_000
        self.pre = {}
        for j, s in enumerate(strs):
            if self.full:
                for L in range(min_overlap, len(s) + 1):
                    self.pre.setdefault(s[:L], []).append(j)
            elif len(s) >= min_overlap:
                self.pre.setdefault(s[:min_overlap], []).append(j)

    def hits(self, p, strand=0):
        """(record, length, strand, flags) of one strand of pattern p, by (length descending, record ascending)"""
        q = (revcomp(p) if strand else p).upper()
        m, out = len(q), []
        for L in range(min(m, self.longest), self.min_overlap - 1, -1):
            suf = q[m - L:]
            if self.full:
                js = self.pre.get(suf, ())
            else:
                js = [j for j in self.pre.get(suf[:self.min_overlap], ()) if self.strs[j][:L] == suf]
            for j in js:
                out.append((j, L, strand, (CONTAINS if L == len(self.strs[j]) else 0) | (WHOLE if L == m else 0)))
        return out

    def both(self, p):
        return self.hits(p, 0) + self.hits(p, 1)


def longest_of(hits):
    """the reduction of DEBWT_FM_OVERLAP_LONGEST on a list in the documented order"""
    seen, out = set(), []
    for h in hits:
        if (h[2], h[0]) not in seen:
            seen.add((h[2], h[0]))
            out.append(h)
    return out


def rand_dna(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def synthetic_reads(seed=20240613):
    """Reads of 80 b at every 7th position of a 3 kb random genome, 9 exact duplicates, three records that are the first
    40 b of other reads, periodic records, one 400 b record; shuffled.  Every record is at least 40 b."""
    rng = np.random.default_rng(seed)
    g = rand_dna(rng, 3000)
    reads = [g[a:a + 80] for a in range(0, 3000 - 80 + 1, 7)]
    n0 = len(reads)
    reads += [reads[int(x)] for x in rng.integers(0, n0, 9)]
    reads += [reads[int(x)][:40] for x in rng.integers(0, n0, 3)]
    reads += ["AC" * 25, "AC" * 30, "CA" * 25, "A" * 40, "A" * 50]
    reads.append(g[1001:1401])
    order = rng.permutation(len(reads))
    return [reads[int(i)] for i in order]


def extra_queries(strs, min_overlap, seed=99):
    """lower case, an N in the middle, an N at the end, empty, shorter than min_overlap, one longer than every record
    whose tail is a whole record, a random string"""
    rng = np.random.default_rng(seed)
    r = strs[3]
    mid = len(r) // 2
    short = strs[5][-(min_overlap - 1):] if min_overlap > 1 else ""
    return [strs[1].lower(), r[:mid] + "N" + r[mid + 1:], strs[2][:-1] + "N", "", short,
            rand_dna(rng, max(len(s) for s in strs) + 50) + strs[4], rand_dna(rng, 120)]


def codes(strs):
    lut = {c: i for i, c in enumerate("ACGT")}
    return [np.array([lut[c] for c in s], dtype=np.uint8) for s in strs]
