"""Definition 14 written out on the CPU: the compacted de Bruijn graph of a collection over both strands, twice.

brute(strs, k)   dictionaries over the records' strings and their reverse complements.
from_esa(E, k)   the same answer from esa_ref.Esa by interval rules: the present nodes are the intervals of Definition 13,
                 the mate of a node is the interval a backward search of its reverse complement ends in, and the oriented
                 edge strings come from the symbols in front of the rows, each with its mirror.
fold(G, k, present)  a Definition 13 answer on the doubled collection D with each mirror pair folded into one record; equal
                 to Definition 14 where that has no hairpin.

Both builders hand the present nodes (in string order, which is row order), their mates, occurrence counts and forward
edge strings to one assemble(), which numbers the oriented nodes (a present node v is v, the mirror of an unmated v is
N + v, the mirror of a mated v is its mate), applies the link rule, walks chains and cycles, chooses the reported
orientation of every pair and maps the edges.  It asserts that no unitig holds a node and its mirror, that every edge
string that is no member link leaves a last node and enters a first node, and that the edge list is closed under
(x, y) -> (y ^ 1, x ^ 1).  facts() asserts facts 1 to 3.  Nothing here calls the library."""
import collections

import numpy as np

import cdbg_ref as CR
import fm_definition as F

COUNTING = CR.COUNTING + ("present", "mated", "hairpins")


def rc_codes(a):
    return (3 - np.asarray(a, dtype=np.uint8))[::-1].copy()


def doubled(records):
    """D = (S_0, rc S_0, S_1, rc S_1, ...) as code arrays"""
    out = []
    for r in records:
        out += [np.asarray(r, dtype=np.uint8), rc_codes(r)]
    return out


def assemble(N, mate, occ, fwd):
    """N present nodes, mate[v] (-1: the reverse complement does not occur), occ[v], fwd = the forward edge strings of S
    as (p, w) pairs of present nodes -> (reported, edges, counts): reported = [(oriented ids, circular)] ascending by w*,
    edges = sorted (from, to) with from = 2a + oa."""
    def mirror(x):
        if x >= N:
            return x - N
        return mate[x] if mate[x] >= 0 else N + x

    ids = list(range(N)) + [N + v for v in range(N) if mate[v] < 0]
    for x in ids:
        assert mirror(mirror(x)) == x and mirror(x) != x
    succ, pred = collections.defaultdict(set), collections.defaultdict(set)
    for p, w in fwd:
        for x, y in ((p, w), (mirror(w), mirror(p))):
            succ[x].add(y)
            pred[y].add(x)
    oriented = sorted((x, y) for x in succ for y in succ[x])
    link, hairpins = {}, 0
    for y in ids:
        if len(pred[y]) == 1:
            (x,) = pred[y]
            if len(succ[x]) == 1 and x != y:
                if x == mirror(y):
                    hairpins += 1
                else:
                    link[y] = x
    nxt = {}
    for y, x in link.items():
        assert x not in nxt
        nxt[x] = y
    for y, x in link.items():                              # links are closed under the mirror
        assert link.get(mirror(x)) == mirror(y)
    chains, seen = [], set()
    for v in ids:
        if v not in link:
            nodes = [v]
            while nodes[-1] in nxt:
                nodes.append(nxt[nodes[-1]])
            seen.update(nodes)
            chains.append((nodes, False))
    for v in ids:                                          # what is left are cycles: ascending ids meet the lowest first
        if v not in seen:
            nodes = [v]
            while nxt[nodes[-1]] != v:
                nodes.append(nxt[nodes[-1]])
            assert not seen.intersection(nodes)
            seen.update(nodes)
            chains.append((nodes, True))
    assert len(seen) == len(ids)
    owner = {}
    for i, (nodes, _) in enumerate(chains):
        for z in nodes:
            owner[z] = i
    reported = []
    for i, (nodes, circular) in enumerate(chains):
        members = set(nodes)
        assert not any(mirror(z) in members for z in nodes), "a unitig holds a node and its mirror"
        j = owner[mirror(nodes[-1])]
        other = chains[j][0]
        assert j != i and chains[j][1] == circular and set(other) == {mirror(z) for z in nodes}
        if not circular:
            assert other == [mirror(z) for z in reversed(nodes)]
        if min(nodes) < min(other):
            assert min(nodes) < N, "the pair has a member that occurs in S"
            reported.append((nodes, circular))
    assert 2 * len(reported) == len(chains)
    reported.sort(key=lambda c: min(c[0]))
    first, last, member = {}, {}, set()
    for a, (nodes, circular) in enumerate(reported):
        assert not circular or nodes[0] == min(nodes)
        flip = [mirror(z) for z in reversed(nodes)]        # the other orientation: for a cycle, cut where the mirror is cut
        for o, path in ((0, nodes), (1, flip)):
            first[path[0]], last[path[-1]] = 2 * a + o, 2 * a + o
            member.update(zip(path, path[1:]))
    edges = []
    for x, y in oriented:
        if (x, y) in member:
            continue
        assert x in last and y in first, "an edge string leaves a last node and enters a first node"
        edges.append((last[x], first[y]))
    assert len(set(edges)) == len(edges)
    edges.sort()
    assert sorted((y ^ 1, x ^ 1) for x, y in edges) == edges, "the edge list is closed under the mirror"
    links = sum(len(c[0]) - 1 for c in reported)
    assert len(oriented) == 2 * links + len(edges)                                            # fact 2
    mated = sum(1 for v in range(N) if mate[v] >= 0)
    assert mated % 2 == 0
    counts = {"nodes": N - mated // 2, "edge_strings": len(oriented), "unitigs": len(reported),
              "circular": sum(1 for c in reported if c[1]), "links": links, "edges": len(edges),
              "longest_nodes": max([len(c[0]) for c in reported], default=0), "present": N, "mated": mated,
              "hairpins": hairpins}
    assert sum(len(c[0]) for c in reported) == counts["nodes"]                                # fact 1, by the ids
    return reported, edges, counts


def _pack(k, N, mate, occ, row_lo, word, reported, edges, counts):
    def spell(z):
        return word(z) if z < N else F.revcomp(word(z - N))

    def both(z):
        if z >= N:
            return occ[z - N]
        return occ[z] + (occ[mate[z]] if mate[z] >= 0 else 0)
    un = np.zeros(len(reported), dtype=CR.UNITIG_DTYPE)
    parts, off = [], 0
    for i, (nodes, circular) in enumerate(reported):
        s = spell(nodes[0]) + "".join(spell(z)[-1] for z in nodes[1:])
        for j, z in enumerate(nodes):
            assert s[j:j + k] == spell(z)
        un[i] = (row_lo[min(nodes)], off, sum(both(z) for z in nodes), len(nodes), CR.CIRCULAR if circular else 0)
        parts.append(s)
        off += len(s)
    seq = np.frombuffer("".join(parts).encode(), dtype=np.uint8).copy()
    ed = np.zeros(len(edges), dtype=CR.EDGE_DTYPE)
    for i, (a, b) in enumerate(edges):
        ed[i] = (a, b)
    counts = dict(counts, seq_bytes=off)
    assert set(counts) == set(COUNTING)
    return CR.Cdbg(k, un, seq, ed, counts)


def brute(strs, k):
    """the definition with dictionaries; row_lo is not known here and stays 0"""
    assert k % 2 == 1
    occ = collections.Counter()
    estr = set()
    for s in strs:
        for i in range(len(s) - k + 1):
            occ[s[i:i + k]] += 1
        for i in range(len(s) - k):
            estr.add(s[i:i + k + 1])
    words = sorted(occ)
    at = {w: i for i, w in enumerate(words)}
    mate = [at.get(F.revcomp(w), -1) for w in words]
    fwd = [(at[e[:k]], at[e[1:]]) for e in sorted(estr)]
    o = [occ[w] for w in words]
    reported, edges, counts = assemble(len(words), mate, o, fwd)
    assert counts["nodes"] == len({min(w, F.revcomp(w)) for w in words})                      # fact 1
    assert counts["edge_strings"] == len(estr | {F.revcomp(e) for e in estr})                 # fact 2
    G = _pack(k, len(words), mate, o, [0] * len(words), lambda v: words[v], reported, edges, counts)
    facts(G, strs)
    return G


def from_esa(E, k, max_lcp=0):
    """the interval rules of Definition 14 on the stored arrays of E (capped at max_lcp, which must be 0 or above k)"""
    assert k >= 1 and k % 2 == 1 and (max_lcp == 0 or k + 1 <= max_lcp)
    n, sa, d, sym = E.n, E.sa, E.d, E.sym
    lcp = E.lcp(max_lcp).astype(np.int64)
    L = sym[(sa - 1) % n]
    starts = np.nonzero(lcp < k)[0]
    ends = np.concatenate([starts[1:], [n]])
    isnode = d[starts] >= k
    lo, hi = starts[isnode], ends[isnode]
    N = len(lo)
    C = np.array([int(np.count_nonzero(sym < c)) for c in range(4)], dtype=np.int64)
    cocc = np.stack([np.concatenate([[0], np.cumsum(L == c)]) for c in range(4)]).astype(np.int64)
    # mates: every node searches its reverse complement backward, reading itself forward and stepping with the complement
    a, b = np.zeros(N, dtype=np.int64), np.full(N, n, dtype=np.int64)
    pos = sa[lo]
    for j in range(k):
        c = 3 - sym[pos + j].astype(np.int64)
        a, b = C[c] + cocc[c, a], C[c] + cocc[c, b]
    at = {int(r): v for v, r in enumerate(lo.tolist())}
    mate = []
    for v in range(N):
        if b[v] > a[v]:
            u = at[int(a[v])]
            assert hi[u] == b[v] and u != v
            mate.append(u)
        else:
            mate.append(-1)
    fwd = []
    for w in range(N):
        i, e = int(lo[w]), int(hi[w])
        for c in range(4):
            if cocc[c, e] - cocc[c, i]:
                row = int(C[c] + cocc[c, i])
                piece = int(np.searchsorted(starts, row, side="right")) - 1
                p = at[int(starts[piece])]
                assert row < hi[p], "the row of a left extension lies in a node"
                fwd.append((p, w))
    occ = (hi - lo).tolist()
    reported, edges, counts = assemble(N, mate, occ, fwd)

    def word(v):
        p = int(sa[lo[v]])
        return "".join(F.ACGT[c] for c in sym[p:p + k].tolist())
    G = _pack(k, N, mate, occ, lo.tolist(), word, reported, edges, counts)
    if E.records is not None:
        facts(G, F.strings(E.records))
    return G


def facts(G, strs):
    """facts 1 to 3 of Definition 14 from the strings"""
    k, un = G.k, G.unitigs
    kmers, estr = set(), set()
    for s in strs:
        for i in range(len(s) - k + 1):
            kmers.add(min(s[i:i + k], F.revcomp(s[i:i + k])))
        for i in range(len(s) - k):
            estr.update((s[i:i + k + 1], F.revcomp(s[i:i + k + 1])))
    nodes = int(un["nodes"].astype(np.int64).sum())
    assert nodes == len(kmers) == G.counts["nodes"]                                           # 1
    assert 2 * (nodes - len(un)) + len(G.edges) == len(estr) == G.counts["edge_strings"]      # 2
    assert int(un["kmer_count"].sum()) == sum(max(0, len(s) - k + 1) for s in strs)           # 3
    assert len(G.seq) == nodes + len(un) * (k - 1) == G.counts["seq_bytes"]
    off = np.concatenate([[0], np.cumsum(un["nodes"].astype(np.int64) + k - 1)])[:-1]
    assert np.array_equal(un["seq_offset"].astype(np.int64), off)
    assert (np.diff(un["row_lo"].astype(np.int64)) > 0).all() or not un["row_lo"].any()


def fold(G, k, present):
    """A Definition 13 answer on the doubled collection -> Definition 14's unitigs, strings and edges.  present: the set of
    k-mers that occur in S.  The linear unitigs are paired by reverse-complement string, the circular ones by k-mer set;
    the member of a pair that holds w*, the lowest k-mer of the pair that occurs in S (string order is row order), is
    reported, a cycle turned so that it starts at w*; pairs are numbered by ascending w*, and the edges are mapped through
    the pairing.  Returns (records as (string, nodes, kmer_count, circular), edges); occ in D of a k-mer is occ W + occ rc W
    in S, so kmer_count is Definition 14's."""
    strs = G.strings()
    kml = [[s[i:i + k] for i in range(len(s) - k + 1)] for s in strs]
    kms = [frozenset(x) for x in kml]
    circ = [bool(u["flags"] & CR.CIRCULAR) for u in G.unitigs]
    by_str = {s: i for i, s in enumerate(strs) if not circ[i]}
    by_set = {kms[i]: i for i in range(len(strs)) if circ[i]}
    partner = []
    for i, s in enumerate(strs):
        j = by_set[frozenset(F.revcomp(w) for w in kms[i])] if circ[i] else by_str[F.revcomp(s)]
        assert j != i
        partner.append(j)
    star = [min([w for w in kms[i] if w in present], default="~") for i in range(len(strs))]
    keep = sorted((i for i in range(len(strs)) if star[i] < star[partner[i]]), key=lambda i: star[i])
    assert 2 * len(keep) == len(strs)
    oid = {}
    for a, i in enumerate(keep):
        oid[i], oid[partner[i]] = 2 * a, 2 * a + 1
    recs = []
    for i in keep:
        s, u = strs[i], G.unitigs[i]
        if circ[i]:
            j = kml[i].index(star[i])
            turned = kml[i][j:] + kml[i][:j]
            s = turned[0] + "".join(w[-1] for w in turned[1:])
        recs.append((s, int(u["nodes"]), int(u["kmer_count"]), circ[i]))
    edges = sorted({(oid[int(e["from"])], oid[int(e["to"])]) for e in G.edges})
    return recs, edges


def kmers_of(strs, k):
    return {s[i:i + k] for s in strs for i in range(len(s) - k + 1)}


def folded(G):
    """a Definition 14 answer in the form fold() gives"""
    recs = [(s, int(u["nodes"]), int(u["kmer_count"]), bool(u["flags"] & CR.CIRCULAR))
            for s, u in zip(G.strings(), G.unitigs)]
    return recs, [(int(e["from"]), int(e["to"])) for e in G.edges]


def same_graph(a, b, rows=True):
    CR.same_graph(a, b, rows)
