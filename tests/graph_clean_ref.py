"""Shared by the graph cleaning tests: definition 6 of include/debwt_hip.h (tip clipping and bubble popping over a
string graph) taken literally -- every phase reads one snapshot of the alive nodes and applies its removals together --
and the read set the tests share: a 2 kb tiling with five end-error reads and six reads of a second allele."""
import numpy as np

from overlap_ref import rand_dna

CLIPPED, POPPED = 3, 4


def _snapshot(state, lists):
    """(out, inn): per alive node the alive targets and the alive sources, one entry per edge as given"""
    n = len(state)
    out, inn = [[] for _ in range(n)], [[] for _ in range(n)]
    for u, l in enumerate(lists):
        if state[u] != 0:
            continue
        for e in l:
            v = e[0]
            if state[v] == 0:
                out[u].append(v)
                inn[v].append(u)
    return out, inn


def _tip_chains(out, inn, max_tip):
    """the chains of the tip edges that a junction with at least one other edge clips, in one direction"""
    found = []
    for w, l in enumerate(out):
        if len(l) < 2:
            continue
        chains = []
        for x in l:
            c, chain = x, []
            while True:
                if len(inn[c]) != 1 or len(chain) == max_tip:
                    chain = None
                    break
                chain.append(c)
                if len(out[c]) == 0:
                    break
                if len(out[c]) != 1:
                    chain = None
                    break
                c = out[c][0]
            chains.append(chain)
        if any(c is None for c in chains):
            found += [c for c in chains if c is not None]
    return found


def _branch(out, inn, w, x, max_bubble):
    """(chain, z) of the simple branch that starts with the edge w -> x, or None"""
    c, chain = x, []
    while True:
        if len(inn[c]) >= 2:
            return (chain, c) if chain and c != w else None
        if len(inn[c]) == 0 or len(out[c]) != 1 or len(chain) == max_bubble:
            return None
        chain.append(c)
        c = out[c][0]


def _bubble_chains(out, inn, max_bubble, mirrored):
    """the chains that lose their group"""
    found = []
    for w, l in enumerate(out):
        if len(l) < 2:
            continue
        groups = {}
        for x in l:
            b = _branch(out, inn, w, x, max_bubble)
            if b is not None:
                chain, z = b
                key = min(v >> 1 if mirrored else v for v in chain)
                groups.setdefault(z, []).append((-len(chain), key, chain))
        for g in groups.values():
            if len(g) < 2:
                continue
            g.sort(key=lambda t: t[:2])
            if g[0][:2] != g[1][:2]:
                found += [t[2] for t in g[1:]]
    return found


def clean_full(state, lists, max_tip, max_bubble, max_rounds, mirrored=False):
    """definition 6.  lists: per node a list of (target, ...) tuples.  Returns a dict: state (list), keep (per node a list
    of bools, one per edge), rounds, tips, tip_nodes, bubbles, bubble_nodes."""
    assert (max_tip or max_bubble) and max_rounds
    state = [int(s) for s in state]
    st = dict(rounds=0, tips=0, tip_nodes=0, bubbles=0, bubble_nodes=0)
    while st["rounds"] < max_rounds:
        st["rounds"] += 1
        out, inn = _snapshot(state, lists)
        tips = _tip_chains(out, inn, max_tip) + _tip_chains(inn, out, max_tip)
        for chain in tips:
            for v in chain:
                assert state[v] == 0, "a node in two tips"
                state[v] = CLIPPED
        out, inn = _snapshot(state, lists)
        pops = _bubble_chains(out, inn, max_bubble, mirrored)
        for chain in pops:
            for v in chain:
                assert state[v] == 0, "a node in two popped chains"
                state[v] = POPPED
        st["tips"] += len(tips)
        st["tip_nodes"] += sum(len(c) for c in tips)
        st["bubbles"] += len(pops)
        st["bubble_nodes"] += sum(len(c) for c in pops)
        if not tips and not pops:
            break
    st["state"] = state
    st["keep"] = [[state[u] == 0 and state[e[0]] == 0 for e in l] for u, l in enumerate(lists)]
    return st


def clean(state, lists, max_tip, max_bubble, max_rounds, mirrored=False):
    """(state_out, lists_out, rounds): the states with CLIPPED and POPPED written in, the edges between alive nodes"""
    r = clean_full(state, lists, max_tip, max_bubble, max_rounds, mirrored)
    return r["state"], [[e for e, k in zip(l, kl) if k] for l, kl in zip(lists, r["keep"])], r["rounds"]


def _subst(s, p):
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + 1) % 4] + s[p + 1:]


def error_reads(seed=7):
    """(g, reads): 60 b reads at every 5th base of a 2 kb string; the reads at 300, 900, 1500 with base 55 substituted and
    those at 500, 1200 with base 4 (end errors: tips); six more reads at 945 .. 995 with base 1000 of the string
    substituted (a second allele: a bubble); shuffled"""
    rng = np.random.default_rng(seed)
    g = rand_dna(rng, 2000)
    reads = []
    for a in range(0, 1941, 5):
        r = g[a:a + 60]
        if a in (300, 900, 1500):
            r = _subst(r, 55)
        if a in (500, 1200):
            r = _subst(r, 4)
        reads.append(r)
    g2 = _subst(g, 1000)
    reads += [g2[a:a + 60] for a in range(945, 996, 10)]
    return g, [reads[int(i)] for i in rng.permutation(len(reads))]


def lists_of(n, pairs):
    """per-node lists of (target, 1) from (source, target) pairs, in the order given"""
    out = [[] for _ in range(n)]
    for u, v in pairs:
        out[u].append((v, 1))
    return out


def _path(*nodes):
    return list(zip(nodes, nodes[1:]))


def corner_graphs():
    """name -> (state, lists, max_tip, max_bubble, max_rounds, mirrored, expected {node: state written}): one hand-made
    graph of at most 20 nodes per corner of definition 6"""
    c = {}

    def add(name, n, pairs, expect, T=3, B=4, R=8, mirrored=False, state=None):
        c[name] = (state or [0] * n, lists_of(n, pairs), T, B, R, mirrored, expect)

    main = _path(*range(10))
    add("tips_1_T_T+1", 18, main + [(1, 10)] + _path(3, 11, 12, 13) + _path(5, 14, 15, 16, 17), {10: 3, 11: 3, 12: 3, 13: 3})
    add("fork_all_tips", 5, _path(0, 1, 2, 3) + [(2, 4)], {})
    add("tip_both_ways", 11, _path(*range(9)) + [(4, 9), (10, 4)], {9: 3, 10: 3})
    add("bubble_unequal", 7, [(0, 1)] + _path(1, 2, 3, 5) + _path(1, 4, 5) + [(5, 6)], {4: 4})
    add("bubble_by_key", 7, [(0, 1)] + _path(1, 3, 5) + _path(1, 2, 5) + [(5, 6)], {3: 4})
    tie = _path(0, 2, 4) + _path(0, 3, 4)
    add("mirrored_tie", 6, tie, {}, mirrored=True)
    add("unmirrored_no_tie", 6, tie, {3: 4})
    add("three_branches", 9, [(0, 1)] + _path(1, 2, 3, 7) + _path(1, 4, 7) + _path(1, 5, 6, 7) + [(7, 8)], {4: 4, 5: 4, 6: 4})
    add("three_branches_tie", 10, [(0, 2)] + _path(2, 4, 1) + _path(2, 5, 1) + _path(2, 6, 1) + [(1, 8)], {}, T=0, mirrored=True)
    add("branch_B_and_B+1", 13, _path(0, 1, 2, 3, 4, 11) + _path(0, 5, 6, 7, 8, 9, 11) + _path(0, 10, 11) + [(11, 12)], {10: 4})
    add("branch_into_w", 7, _path(6, 5, 4, 3, 0) + _path(0, 1, 0) + _path(0, 2, 0), {})
    add("cycle_off_junction", 14, _path(*range(10)) + [(5, 10)] + _path(10, 11, 12, 13, 10), {}, B=8)
    add("junction_on_cycle", 9, _path(0, 1, 2, 0) + _path(0, 3, 4, 5, 6, 7, 8), {}, T=5, B=8)
    late = [(0, 1), (0, 5)] + _path(5, 6, 7, 8) + [(1, 2), (1, 3), (2, 4), (3, 4)]
    add("tip_after_pop", 9, late, {3: 4, 1: 3, 2: 3, 4: 3})
    add("tip_after_pop_one_round", 9, late, {3: 4}, R=1)
    add("dead_nodes", 10, [(0, 3)] + _path(3, 4, 6, 8) + _path(3, 7, 8) + [(8, 9)], {7: 4}, state=[0, 1, 2, 0, 0, 2, 0, 0, 0, 0])
    add("double_edge", 6, _path(0, 1, 2, 3, 4) + [(1, 2), (1, 5)], {5: 3})
    return c


def random_graph(rng):
    """(state, lists): 30 to 300 nodes, out-degree 0 to 3, no edge from a node to itself; half of them a backbone of paths
    with tips, bubbles and stray edges, the others random targets throughout"""
    n = int(rng.integers(30, 301))
    out = [[] for _ in range(n)]

    def link(u, v):
        if u != v and len(out[u]) < 3 and v not in out[u]:
            out[u].append(v)

    if rng.random() < 0.5:
        for u in range(n):
            for v in rng.integers(0, n, size=int(rng.choice(4, p=[0.2, 0.55, 0.2, 0.05]))):
                link(u, int(v))
    else:
        order = [int(x) for x in rng.permutation(n)]
        back = order[:n // 2]
        for u, v in zip(back, back[1:]):
            if rng.random() < 0.97:
                link(u, v)
        spare = order[n // 2:]
        while len(spare) > 10:
            k = int(rng.integers(1, 8))
            chain, spare = spare[:k], spare[k:]
            a = int(rng.integers(0, len(back) - 1))
            kind = int(rng.integers(0, 4))
            for u, v in zip(chain, chain[1:]):
                link(u, v)
            if kind != 1:
                link(back[a], chain[0])                            # a forward tip, or the way into a bubble
            if kind != 0:
                link(chain[-1], back[min(len(back) - 1, a + int(rng.integers(1, 6)))])   # a backward tip, or the way out
        for _ in range(int(rng.integers(0, 6))):
            link(int(rng.integers(0, n)), int(rng.integers(0, n)))
    state = [0] * n
    return state, [[(v, 1) for v in l] for l in out]


def random_mirrored_graph(rng):
    """(state, lists) over nodes 2r + o: a random_graph() on the + nodes, a few edges across the strands, and the
    mirror v^1 -> u^1 of every edge u -> v"""
    state, lists = random_graph(rng)
    n = 2 * len(state)
    have = {(2 * u, 2 * v) for u, l in enumerate(lists) for v, _ in l}
    for _ in range(int(rng.integers(0, 5))):
        have.add((int(rng.integers(0, n)), int(rng.integers(0, n))))
    have |= {(v ^ 1, u ^ 1) for u, v in have}
    return [0] * n, lists_of(n, sorted(p for p in have if p[0] != p[1]))


def long_chains(n=70000, every=50, max_tip=3):
    """(state, lists): a backbone with a dead-end chain of 1 .. max_tip + 1 nodes at every 50th node, about n nodes"""
    pairs, nxt, u = [], 1, 0
    while nxt < n - max_tip - 2:
        for k in range(every):
            pairs.append((u, nxt))
            u, nxt = nxt, nxt + 1
        w = u
        for k in range(1 + (u // every) % (max_tip + 1)):
            pairs.append((w, nxt))
            w, nxt = nxt, nxt + 1
    return [0] * nxt, lists_of(nxt, pairs)
