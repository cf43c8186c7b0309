"""Definition 13 written out on the CPU: the compacted de Bruijn graph of a collection, forward strand, twice.

brute(strs, k)   dictionaries over the records' strings: every k-mer is a node, every (k+1)-mer an edge string.
from_esa(E, k)   the same answer from esa_ref.Esa by the interval rules of the definition: nodes are the row intervals
                 [i, e) with lcp[i] < k <= d(sa[i]), out() counts the rows that begin a (k+1)-interval, in() and the
                 predecessors come from the symbols in front of the rows.

Both hand their nodes (in string order, which is row order), their occurrence counts, out-degrees and predecessor lists
to one assemble(), which applies the link rule, walks the chains and cycles and numbers unitigs and edges.  Nothing here
calls the library.  facts() asserts the three facts of the definition and the edge property."""
import collections

import numpy as np

import fm_definition as F

CIRCULAR = 1
UNITIG_DTYPE = np.dtype([("row_lo", "<u8"), ("seq_offset", "<u8"), ("kmer_count", "<u8"), ("nodes", "<u4"), ("flags", "<u4")])
EDGE_DTYPE = np.dtype([("from", "<u4"), ("to", "<u4")])
assert UNITIG_DTYPE.itemsize == 32 and EDGE_DTYPE.itemsize == 8
COUNTING = ("nodes", "edge_strings", "unitigs", "circular", "links", "edges", "longest_nodes", "seq_bytes")


class Cdbg:
    """unitigs (UNITIG_DTYPE), seq (uint8, ASCII), edges (EDGE_DTYPE), counts (the counting fields of the statistics)"""

    def __init__(self, k, unitigs, seq, edges, counts):
        self.k, self.unitigs, self.seq, self.edges, self.counts = k, unitigs, seq, edges, counts

    def strings(self):
        s = self.seq.tobytes().decode()
        return [s[int(u["seq_offset"]):int(u["seq_offset"]) + int(u["nodes"]) + self.k - 1] for u in self.unitigs]

    def sizes(self):
        return len(self.unitigs), len(self.seq), len(self.edges)


def assemble(occ, outdeg, preds):
    """occ[v], outdeg[v], preds[v] (the nodes with an edge string into v) of nodes 0 .. N - 1 in string order ->
    (chains, edges, links): chains = [(node list, circular)] ascending by first node, edges = sorted (from, to) pairs
    of chain numbers.  Asserts the edge property on the way."""
    N = len(occ)
    link = [-1] * N
    for v in range(N):
        if len(preds[v]) == 1:
            u = preds[v][0]
            if outdeg[u] == 1 and u != v:
                link[v] = u
    nxt = [-1] * N
    for v, u in enumerate(link):
        if u >= 0:
            assert nxt[u] < 0
            nxt[u] = v
    chains, seen = [], [False] * N
    for v in range(N):                                     # chains that have a first node
        if link[v] < 0:
            nodes = [v]
            while nxt[nodes[-1]] >= 0:
                nodes.append(nxt[nodes[-1]])
            for w in nodes:
                seen[w] = True
            chains.append((nodes, False))
    cut = set()
    for v in range(N):                                     # what is left are cycles: v ascending meets the lowest node first
        if not seen[v]:
            nodes = [v]
            while nxt[nodes[-1]] != v:
                nodes.append(nxt[nodes[-1]])
            for w in nodes:
                assert not seen[w]
                seen[w] = True
            chains.append((nodes, True))
            cut.add(v)
    chains.sort(key=lambda c: c[0][0])
    first = {c[0][0]: i for i, c in enumerate(chains)}
    last = {c[0][-1]: i for i, c in enumerate(chains)}
    edges, links = [], 0
    for v in range(N):
        for u in preds[v]:
            if link[v] == u and v not in cut:
                links += 1
                continue
            assert u in last and v in first, "an edge string leaves a last node and enters a first node"
            edges.append((last[u], first[v]))
    assert len(set(edges)) == len(edges)
    return chains, sorted(edges), links


def _pack(k, chains, edges, links, occ, outdeg, row_lo, spell):
    un = np.zeros(len(chains), dtype=UNITIG_DTYPE)
    parts, off = [], 0
    for i, (nodes, circular) in enumerate(chains):
        s = spell(nodes[0]) + "".join(spell(v)[-1] for v in nodes[1:])
        assert len(s) == len(nodes) + k - 1
        un[i] = (row_lo[nodes[0]], off, sum(occ[v] for v in nodes), len(nodes), CIRCULAR if circular else 0)
        parts.append(s)
        off += len(s)
    seq = np.frombuffer("".join(parts).encode(), dtype=np.uint8).copy()
    ed = np.zeros(len(edges), dtype=EDGE_DTYPE)
    for i, (a, b) in enumerate(edges):
        ed[i] = (a, b)
    counts = {"nodes": len(occ), "edge_strings": int(sum(outdeg)), "unitigs": len(chains),
              "circular": sum(1 for c in chains if c[1]), "links": links, "edges": len(edges),
              "longest_nodes": max([len(c[0]) for c in chains], default=0), "seq_bytes": off}
    assert counts["edge_strings"] == links + len(edges)
    return Cdbg(k, un, seq, ed, counts)


def brute(strs, k):
    """the definition with dictionaries; row_lo is not known here and stays 0"""
    occ = collections.Counter()
    estr = set()
    for s in strs:
        for i in range(len(s) - k + 1):
            occ[s[i:i + k]] += 1
        for i in range(len(s) - k):
            estr.add(s[i:i + k + 1])
    words = sorted(occ)
    at = {w: i for i, w in enumerate(words)}
    preds = [[] for _ in words]
    outdeg = [0] * len(words)
    for e in sorted(estr):                                 # sorted: the predecessors of v by ascending first base
        outdeg[at[e[:k]]] += 1
        preds[at[e[1:]]].append(at[e[:k]])
    chains, edges, links = assemble([occ[w] for w in words], outdeg, preds)
    return _pack(k, chains, edges, links, [occ[w] for w in words], outdeg, [0] * len(words), lambda v: words[v])


def from_esa(E, k, max_lcp=0):
    """the interval rules of Definition 13 on the stored arrays of E (capped at max_lcp, which must be 0 or above k)"""
    assert k >= 1 and (max_lcp == 0 or k + 1 <= max_lcp)
    n, sa, d, sym = E.n, E.sa, E.d, E.sym
    lcp = E.lcp(max_lcp).astype(np.int64)
    L = sym[(sa - 1) % n]
    starts = np.nonzero(lcp < k)[0]
    ends = np.concatenate([starts[1:], [n]])
    assert (lcp[d < k] < k).all()
    isnode = d[starts] >= k
    lo, hi = starts[isnode], ends[isnode]
    N = len(lo)
    outrow = ((lcp <= k) & (d >= k + 1)).astype(np.int64)       # r = i has lcp < k, the others of [i, e) have lcp >= k
    cout = np.concatenate([[0], np.cumsum(outrow)])
    outdeg = (cout[hi] - cout[lo]).tolist()
    C = [int(np.count_nonzero(sym < c)) for c in range(4)]
    cocc = [np.concatenate([[0], np.cumsum(L == c)]) for c in range(4)]
    preds = []
    for v in range(N):
        i, e = int(lo[v]), int(hi[v])
        p = []
        for c in range(4):
            if cocc[c][e] - cocc[c][i]:
                row = C[c] + int(cocc[c][i])
                piece = int(np.searchsorted(starts, row, side="right")) - 1
                u = int(np.searchsorted(lo, starts[piece]))
                assert u < N and lo[u] == starts[piece] and row < hi[u], "the row of a left extension lies in a node"
                p.append(u)
        preds.append(p)
    occ = (hi - lo).tolist()
    chains, edges, links = assemble(occ, outdeg, preds)

    def spell(v):
        p = int(sa[lo[v]])
        return "".join(F.ACGT[c] for c in sym[p:p + k].tolist())
    return _pack(k, chains, edges, links, occ, outdeg, lo.tolist(), spell)


def same_graph(a, b, rows=True):
    """two answers agree; rows=False leaves row_lo out (brute does not know it)"""
    names = [x for x in UNITIG_DTYPE.names if rows or x != "row_lo"]
    assert a.sizes() == b.sizes() and a.counts == b.counts
    for x in names:
        assert np.array_equal(a.unitigs[x], b.unitigs[x]), x
    assert np.array_equal(a.seq, b.seq) and np.array_equal(a.edges, b.edges)


def facts(G, E, strs):
    """the three facts of Definition 13 on one answer"""
    k, un = G.k, G.unitigs
    cap = min(k + 1, 4096)
    prof = E.profile(cap)
    nodes = int(un["nodes"].astype(np.int64).sum())
    if k <= 4096:
        assert nodes == prof[k - 1]                                               # 1
    if k + 1 <= 4096:
        assert nodes - len(un) + len(G.edges) == prof[k]                          # 2
    assert int(un["kmer_count"].sum()) == sum(max(0, len(s) - k + 1) for s in strs)   # 3
    assert nodes == G.counts["nodes"] and len(G.seq) == nodes + len(un) * (k - 1)
    off = np.concatenate([[0], np.cumsum(un["nodes"].astype(np.int64) + k - 1)])[:-1]
    assert np.array_equal(un["seq_offset"].astype(np.int64), off)
    assert (np.diff(un["row_lo"].astype(np.int64)) > 0).all() or not un["row_lo"].any()


def n50(lengths):
    """the largest L such that the unitigs of length >= L hold at least half of all bases; 0 without unitigs"""
    total, run = sum(lengths), 0
    for x in sorted(lengths, reverse=True):
        run += x
        if 2 * run >= total:
            return x
    return 0
