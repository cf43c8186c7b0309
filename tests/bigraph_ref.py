"""Shared by the tests of the string graph over both strands: the doubled collection on which string_graph_ref.Graph is
the definition, random strands, definition 4b (oriented unitigs) taken literally, and crafted reads for the corners of
the tail-to-tail search."""
import numpy as np

from overlap_ref import rand_dna, revcomp
from string_graph_ref import DUPLICATE, KEPT, sequences


def doubled(strs):
    """D = (S_0, rc S_0, S_1, rc S_1, ...): record 2r + o is the oriented node (r, o)"""
    out = []
    for s in strs:
        out += [s, revcomp(s)]
    return out


def stranded(strs, seed):
    """each read reverse-complemented with probability 1/2"""
    flip = np.random.default_rng(seed).random(len(strs)) < 0.5
    return [revcomp(s) if f else s for s, f in zip(strs, flip)]


def is_selfrc(state, v):
    return state[v & ~1] == KEPT and state[v | 1] == DUPLICATE


def mirror(state, path, circ):
    """the path reversed with every member ^ 1 (a self-rc read's node is its own mirror); a cycle from its lowest member"""
    m = [v if is_selfrc(state, v) else v ^ 1 for v in reversed(path)]
    if circ:
        k = m.index(min(m))
        m = m[k:] + m[:k]
    return m


def all_unitigs_both(state, lists):
    """the unitigs of definition 4 under the link rule of 4b, mirrors included: [(path, circular)] by first member"""
    n = len(state)
    indeg = [0] * n
    for l in lists:
        for j, _ in l:
            indeg[j] += 1
    nxt, has_in = {}, set()
    for u, l in enumerate(lists):
        if state[u] != KEPT or len(l) != 1:
            continue
        w = l[0][0]
        if w != u and indeg[w] == 1 and w != u ^ 1 and not is_selfrc(state, u) and not is_selfrc(state, w):
            nxt[u] = w
            has_in.add(w)
    found, seen = [], set()
    for u in range(n):
        if state[u] == KEPT and u not in has_in:
            path = [u]
            while path[-1] in nxt:
                path.append(nxt[path[-1]])
            seen.update(path)
            found.append((path, 0))
    for u in range(n):
        if state[u] == KEPT and u not in seen:
            path = [u]
            while nxt[path[-1]] != u:
                path.append(nxt[path[-1]])
            seen.update(path)
            found.append((path, 1))
    found.sort(key=lambda t: t[0][0])
    return found


def unitigs_both(state, lists):
    """definition 4b: of every mirror pair the unitig with the lower first member, by ascending first member"""
    kept = [(p, c) for p, c in all_unitigs_both(state, lists) if not mirror(state, p, c)[0] < p[0]]
    return [p for p, _ in kept], [c for _, c in kept]


def sequences_both(strs, lists, paths, circular):
    """the oriented string of the first member, then each further member's from its overlap on"""
    return sequences(doubled(strs), lists, paths, circular)


def fold_states(strs):
    """the states of the doubled collection as the issue's rule gives them from S alone"""
    out = []
    for r, s in enumerate(strs):
        rc = revcomp(s)
        if any(t == s or t == rc for t in strs[:r]):
            st = DUPLICATE
        elif any(len(t) > len(s) and (s in t or rc in t) for t in strs):
            st = 2
        else:
            st = KEPT
        out += [st, DUPLICATE if s == rc else st]
    return out


def crafted(strs, min_overlap=20, seed=11):
    """strs and reads for the corners: a kept and a contained self-rc read, a reverse-complemented duplicate, an inner
    part of a reverse complement, a read that overlaps its own mirror, tails that are reverse complements for exactly
    min_overlap and for min_overlap - 1 bases, a seed followed by a mismatch, a seed too early in its read.  Returns
    (reads, names): names maps a word to the read's number."""
    rng = np.random.default_rng(seed)
    out, names = list(strs), {}

    def add(name, s):
        names[name] = len(out)
        out.append(s)

    long80 = [i for i, s in enumerate(strs) if len(s) == 80 and strs.index(s) == i and strs.count(s) == 1]
    add("selfrc", "ACGT" * 20)
    add("selfrc_contained", "ACGT" * 15)
    add("rc_duplicate", revcomp(strs[long80[0]]))
    add("rc_inner", revcomp(strs[long80[1]])[10:60])
    half = rand_dna(rng, 12)
    add("own_mirror", rand_dna(rng, 40) + half + revcomp(half))
    t = rand_dna(rng, min_overlap)
    add("tail_a", rand_dna(rng, 60) + t)
    add("tail_b", rand_dna(rng, 60) + revcomp(t))
    t = rand_dna(rng, min_overlap - 1)
    add("short_a", rand_dna(rng, 60) + t)
    add("short_b", rand_dna(rng, 60) + revcomp(t))
    c = rand_dna(rng, 60 + min_overlap + 10)
    w = revcomp(c[-(min_overlap + 10):-min_overlap])
    w = w[:4] + "ACGT"[("ACGT".index(w[4]) + 1) % 4] + w[5:]
    add("mismatch_src", c)
    add("mismatch", rand_dna(rng, 25) + revcomp(c[-min_overlap:]) + w)
    e = rand_dna(rng, 60)
    add("early_src", e)
    add("early", rand_dna(rng, 5) + revcomp(e[-min_overlap:]) + rand_dna(rng, 60))
    return out, names
