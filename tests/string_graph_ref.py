"""Shared by the string graph tests: the definitions of debwt_fm_string_graph, debwt_fm_edges_reduce and debwt_fm_unitigs
taken literally -- substring tests for the states, overlap_ref.Ref and longest_of for the edges, the triple loop for the
reduction, a walk for the unitigs and their sequences -- and the read sets the tests share."""
import numpy as np

from overlap_ref import Ref, longest_of, rand_dna

KEPT, DUPLICATE, CONTAINED = 0, 1, 2


def states(strs):
    """definition 1: duplicate of an earlier record, else a substring of a strictly longer one, else kept"""
    first, out = {}, []
    for i, s in enumerate(strs):
        if s in first:
            out.append(DUPLICATE)
            continue
        first[s] = i
        out.append(CONTAINED if any(len(t) > len(s) and s in t for t in strs) else KEPT)
    return out


def edge_lists(strs, state, min_overlap):
    """definition 2: per record the list of (target, L), by (L descending, target ascending); empty for a record not kept"""
    R = Ref(strs, min_overlap)
    out = []
    for i, s in enumerate(strs):
        if state[i] != KEPT:
            out.append([])
            continue
        hits = [h for h in longest_of(R.hits(s)) if h[0] != i and state[h[0]] == KEPT]
        for j, L, _, _ in hits:
            assert L < min(len(s), len(strs[j])), (i, j, L)
        out.append([(j, L) for j, L, _, _ in hits])
    return out


def reducible(lists, reclen):
    """definition 3 on any lists: per source a list of bools, True for a reducible edge; E is read as it is"""
    have = [set(l) for l in lists]
    out = []
    for i, l in enumerate(lists):
        red = []
        for k, Lik in l:
            red.append(any(j != k and j != i and Lij > Lik and (k, reclen[j] - Lij + Lik) in have[j] for j, Lij in l))
        out.append(red)
    return out


def reduce_lists(lists, reclen):
    red = reducible(lists, reclen)
    return [[e for e, r in zip(l, rl) if not r] for l, rl in zip(lists, red)]


def unitigs(state, lists):
    """definition 4: (list of member lists, list of circular flags), by ascending first record"""
    n = len(state)
    indeg = [0] * n
    for l in lists:
        for j, _ in l:
            indeg[j] += 1
    nxt, has_in = {}, set()
    for u, l in enumerate(lists):
        if state[u] == KEPT and len(l) == 1 and l[0][0] != u and indeg[l[0][0]] == 1:
            nxt[u] = l[0][0]
            has_in.add(l[0][0])
    found, seen = [], set()
    for u in range(n):
        if state[u] == KEPT and u not in has_in:
            path = [u]
            while path[-1] in nxt:
                path.append(nxt[path[-1]])
            seen.update(path)
            found.append((path, 0))
    for u in range(n):                                         # what is left has an incoming link everywhere: cycles
        if state[u] == KEPT and u not in seen:
            path = [u]
            while nxt[path[-1]] != u:
                path.append(nxt[path[-1]])
            seen.update(path)
            found.append((path, 1))
    found.sort(key=lambda t: t[0][0])
    assert sorted(v for p, _ in found for v in p) == [u for u in range(n) if state[u] == KEPT]
    return [p for p, _ in found], [c for _, c in found]


def sequences(strs, lists, paths, circular):
    """definition 5: the first record, then each further one from its overlap on; a circle is cut by its closing overlap"""
    out = []
    for p, c in zip(paths, circular):
        s = strs[p[0]]
        for a, b in zip(p, p[1:]):
            s += strs[b][dict(lists[a])[b]:]
        if c:
            s = s[:len(s) - dict(lists[p[-1]])[p[0]]]
        out.append(s)
    return out


class Graph:
    """everything the definitions give for one read set and min_overlap"""

    def __init__(self, strs, min_overlap):
        self.strs, self.min_overlap = strs, min_overlap
        self.reclen = [len(s) for s in strs]
        self.state = states(strs)
        self.E = edge_lists(strs, self.state, min_overlap)
        self.red = reducible(self.E, self.reclen)
        self.I = [[e for e, r in zip(l, rl) if not r] for l, rl in zip(self.E, self.red)]
        self.paths, self.circular = unitigs(self.state, self.I)
        self.seqs = sequences(strs, self.I, self.paths, self.circular)


def flat(lists):
    """(offsets, list of (record, length)) of per-source lists"""
    offs, edges = [0], []
    for l in lists:
        edges += l
        offs.append(len(edges))
    return offs, edges


def tiling(seed, n, read, step, circle=False):
    """(string, shuffled reads of `read` bases at every `step`-th position); on a circle the reads wrap round"""
    rng = np.random.default_rng(seed)
    g = rand_dna(rng, n)
    if circle:
        reads = [(g + g)[a:a + read] for a in range(0, n, step)]
    else:
        reads = [g[a:a + read] for a in range(0, n - read + 1, step)]
        assert (n - read) % step == 0
    return g, [reads[int(i)] for i in rng.permutation(len(reads))]


def repeat_reads(seed=5):
    """a 2 kb string whose bases 300..500 come again at 1400..1600: the tiling's graph branches at the repeat"""
    rng = np.random.default_rng(seed)
    g = rand_dna(rng, 2000)
    g = g[:1400] + g[300:500] + g[1600:]
    reads = [g[a:a + 60] for a in range(0, 2000 - 60 + 1, 5)]
    return g, [reads[int(i)] for i in rng.permutation(len(reads))]


def sampled_reads(seed=6, n=1000):
    """n reads of 50..100 b from a 4 kb string: variable lengths, containment inside longer reads, duplicates by chance"""
    rng = np.random.default_rng(seed)
    g = rand_dna(rng, 4000)
    out = []
    for _ in range(n):
        m = int(rng.integers(50, 101))
        a = int(rng.integers(0, 4000 - m + 1))
        out.append(g[a:a + m])
    return out
