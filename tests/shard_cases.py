"""Collections for the sharded builds (debwt_multi_build, debwt_amd/sharded.py) and the host-side definition of what
every shard of them must own.

plan(recs, k, G) restates in numpy -- nothing of it is imported from the code under test -- the 4096-bin census of the node
keys, the splitter rule of the C host (multi_host.cpp, shard_thread, step 1), the text slice of every
rank (shard_slice, debwt_hip.hip), the cut of a shard into key ranges under a range cap (cut_ranges, debwt_hip.hip) and
the multi-in blocks every shard owns.  tests/test_shard_cases_ref.py proves on the CPU that the CASES reach the edges the
GPU tests are there for; the GPU tests compare every shard's report with the plan.

CASES: name -> Case.  A case knows its records, its k, the shard counts it runs at and its expected result:
  "naive"   the BWT by definition (oracle.naive_bwt), row symbols compared -- inputs outside the reference's domain
  "golden"  the reference's bytes: sha256 of the manifest, and the stored outputs where the case has them
  "oracle"  oracle.build_bwt, words / '#' rows / '$' row compared
"""
import functools
import hashlib

import numpy as np

from conftest import golden_manifest, golden_outputs, golden_records, outside_domain_cases

SHARD_BINS = 4096
MAX_RANGES = 64                 # key ranges per shard the C host accepts (multi_host.cpp: MAXR)
MIN_RANGE_CAP = 4096            # debwt_set_range_cap refuses less
WORLDS = (2, 3, 8)


# ---- the definition ----------------------------------------------------------------------------------------------

def node_keys(recs, k):
    """(keys, preds) of every main position in text order: key = node << 2 | pred with pred 3 at a record start (the
    symbol that stands at a separator in the packed text), preds = the real predecessor 0..3, or 4 at a record start ('#'
    or '$': one class)."""
    K = k - 1
    keys, preds = [], []
    for x in recs:
        x = np.asarray(x, dtype=np.uint64)
        m = len(x) - K + 1                                   # windows that end at or before the separator
        node = np.zeros(m, dtype=np.uint64)
        for j in range(K):
            node = (node << np.uint64(2)) | x[j:j + m]
        keys.append((node << np.uint64(2)) | np.concatenate([np.array([3], dtype=np.uint64), x[:m - 1]]))
        preds.append(np.concatenate([np.array([4], dtype=np.uint8), x[:m - 1].astype(np.uint8)]))
    return np.concatenate(keys), np.concatenate(preds)


def cut_ranges(hist, lo, hi, cap):
    """Bin bounds of the key ranges of the shard [lo, hi) under a cap of `cap` instances: near-equal ranges of whole bins,
    a range closed before the bin that would lift it above min(cap, per + per / 16); a bin above that is a range of its own."""
    m = int(hist[lo:hi].sum())
    parts = max(1, -(-m // cap))
    per = -(-m // parts)
    limit = min(cap, per + per // 16)
    bounds, acc = [lo], 0
    for b in (lo + np.flatnonzero(hist[lo:hi])).tolist():          # (an empty bin never closes a range)
        h = int(hist[b])
        if acc and acc + h > limit:
            bounds.append(b)
            acc = 0
        acc += h
    bounds.append(hi)
    return bounds


class Plan:
    """What G shards of (recs, k) own, by definition.
    hist[4096]; bins[G + 1]; keys[G]; special[G]: special suffixes the shard owns; rows[G] = keys + special;
    slices[G] = (p0, p1); blocks[G]: sizes of the multi-in blocks of the shard (a node is
    multi-in when it has two or more distinct real predecessors or stands at a record start: DESIGN.md 2, the rule of the
    reference's mergeKmer), ascending; strict[G]: those of them with two or more distinct predecessors when the '#' / '$'
    predecessor counts as one."""

    def ranges(self, cap):
        """Per shard: the bin bounds of its key ranges under debwt_set_range_cap(cap)."""
        return [cut_ranges(self.hist, self.bins[s], self.bins[s + 1], cap) for s in range(self.G)]

    def range_cap(self):
        """A cap (>= MIN_RANGE_CAP) that cuts the fullest shard into 3 to 40 key ranges and no shard into more than
        MAX_RANGES, aiming at 5 ranges; where no cap does (the fullest shard holds too few keys, or too few bins), the
        smallest cap the interface takes.  Returns (cap, ranges of the fullest shard)."""
        full = int(np.argmax(self.keys))
        for t in sorted(range(3, 41), key=lambda t: (abs(t - 5), t)):
            cap = max(MIN_RANGE_CAP, -(-self.keys[full] // t))
            counts = [len(b) - 1 for b in self.ranges(cap)]
            if 3 <= counts[full] <= 40 and max(counts) <= MAX_RANGES:
                return cap, counts[full]
            if cap == MIN_RANGE_CAP and t >= 5:
                break                                        # more parts ask for the same cap
        return MIN_RANGE_CAP, len(self.ranges(MIN_RANGE_CAP)[full]) - 1


def special_census(recs, k):
    """4096-bin census of the special suffixes: the k - 1 suffixes of every record that meet its separator within k - 1
    symbols.  '#' and '$' sort above T, so the suffix of d bases stands behind every node that starts with those d bases:
    its place among the nodes is that of (the d bases, then T up to k - 1 symbols), and the shard that owns that key owns
    its row."""
    K = k - 1
    tails = np.stack([np.asarray(x[len(x) - (K - 1):], dtype=np.int64) for x in recs])       # d = K - 1 bases at the most
    tails = np.concatenate([tails, np.full((len(recs), 6), 3, dtype=np.int64)], axis=1)
    hist = np.zeros(SHARD_BINS, dtype=np.int64)
    for d in range(K):
        six = tails[:, K - 1 - d:K - 1 - d + 6]
        b = np.zeros(len(recs), dtype=np.int64)
        for j in range(6):
            b = b << 2 | six[:, j]
        hist += np.bincount(b, minlength=SHARD_BINS)
    return hist


def census(recs, k):
    """(hist of the node keys, hist of the special suffixes, and of every multi-in node: its bin, its size, whether it is
    multi-in in the strict sense): the part of a plan that does not depend on G."""
    keys, preds = node_keys(recs, k)
    hist = np.bincount((keys >> np.uint64(2 * k - 12)).astype(np.int64), minlength=SHARD_BINS).astype(np.int64)
    nodes, inv, size = np.unique(keys >> np.uint64(2), return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    seen = np.stack([np.bincount(inv[preds == p], minlength=len(nodes)) > 0 for p in range(5)])
    multi_in = (seen[:4].sum(axis=0) >= 2) | seen[4]
    strict = (seen.sum(axis=0) >= 2)[multi_in]
    nbin = (nodes[multi_in] >> np.uint64(2 * k - 14)).astype(np.int64)      # a node has 2k - 2 bits
    return hist, special_census(recs, k), nbin, size[multi_in].astype(np.int64), strict


@functools.lru_cache(maxsize=None)
def _census_of_case(name):
    return census(CASES[name].records(), CASES[name].k)


def plan(recs, k, G, _census_of=None):
    """The plan of G shards of any list of code arrays (CASES go through plan_case, which keeps the census of a case)."""
    if _census_of is None:
        _census_of = census(recs, k)
    hist, sbin, nbin, size, strict = _census_of
    p = Plan()
    p.G, p.k, p.hist = G, k, hist
    p.nrec = len(recs)
    p.n = int(sum(len(r) for r in recs)) + p.nrec
    # splitters: shard s starts at the first bin whose cumulative count reaches total * s / G, never before shard s - 1
    cum = np.concatenate([[0], np.cumsum(hist)])
    bins = [0]
    for s in range(1, G):
        target = int(cum[-1]) * s // G
        b = int(np.searchsorted(cum, target, side="left"))                    # std::lower_bound over cum[0..4096]
        bins.append(min(max(b, bins[-1]), SHARD_BINS))
    bins.append(SHARD_BINS)
    p.bins = bins
    p.keys = [int(cum[bins[s + 1]] - cum[bins[s]]) for s in range(G)]
    # slices: whole text words per rank, the last rank takes the rest
    per = ((p.n // G) >> 5) << 5
    p.slices = [(per * r, p.n if r + 1 == G else per * (r + 1)) for r in range(G)]
    p.special = [int(sbin[bins[s]:bins[s + 1]].sum()) for s in range(G)]
    p.rows = [a + b for a, b in zip(p.keys, p.special)]
    p.blocks, p.strict = [], []
    for s in range(G):
        own = (nbin >= bins[s]) & (nbin < bins[s + 1])
        p.blocks.append(np.sort(size[own]))
        p.strict.append(np.sort(size[own & strict]))
    return p


@functools.lru_cache(maxsize=None)
def plan_case(name, G):
    c = CASES[name]
    return plan(c.records(), c.k, G, _census_of_case(name))


# ---- the collections ---------------------------------------------------------------------------------------------

def _rand(rng, m):
    return rng.integers(0, 4, size=int(m)).astype(np.uint8)


def blocks_first_middle_last():
    """Three units of 40 bases that start AAACCC, GACGAC and TTTGGG, 2600, 700 and 2300 copies of them in shuffled order
    with random spacers of 3..8 bases between the copies, and one record of 300 bases: at k = 32 the node a unit starts
    with is a multi-in block of as many rows as the unit has copies -- above the LDS capacity in the first AND in the last
    shard, 257..2048 rows in a middle one -- and the nodes that start one or two spacer bases before a unit spread blocks
    of a few dozen to a few hundred rows over the whole key space."""
    rng = np.random.default_rng(12)
    units = [_rand(rng, 40) for _ in range(3)]
    for u, head in zip(units, ([0, 0, 0, 1, 1, 1], [2, 0, 1, 2, 0, 1], [3, 3, 3, 2, 2, 2])):
        u[:6] = head
    order = np.repeat(np.arange(3), [2600, 700, 2300])
    rng.shuffle(order)
    parts = []
    for u in order:
        parts.append(units[int(u)])
        parts.append(_rand(rng, rng.integers(3, 9)))
    return [np.concatenate(parts), _rand(rng, 300)]


def deep_ties():
    """tests/test_gpu_parity.py::test_hip_large_blocks_with_long_ties with the core starting TTTGGG: 4200 copies of a
    36-base core inside 70 exact copies of a 2400-base segment -- a block above the LDS capacity whose rows tie beyond the
    first two SP windows, owned by the LAST shard."""
    rng = np.random.default_rng(9)
    core = _rand(rng, 36)
    core[:6] = [3, 3, 3, 2, 2, 2]
    seg_parts = []
    for _ in range(60):
        seg_parts.append(core)
        seg_parts.append(_rand(rng, rng.integers(2, 6)))
    seg = np.concatenate(seg_parts)
    parts = []
    for _ in range(70):
        parts.append(seg)
        parts.append(_rand(rng, rng.integers(40, 90)))
    return [np.concatenate(parts), _rand(rng, 300)]


def periodic():
    """tests/test_gpu_parity.py::test_hip_periodic_stretches_pivot_rounds, (seed, runs, maxrun) = (5, 40, 9000): runs of one
    symbol and tandem repeats thousands of symbols long."""
    rng = np.random.default_rng(5)
    runs, maxrun = 40, 9000
    parts = []
    for _ in range(runs):
        parts.append(np.full(int(rng.integers(200, maxrun)), int(rng.integers(0, 4)), dtype=np.uint8))
        parts.append(np.tile(_rand(rng, rng.integers(2, 7)), int(rng.integers(50, maxrun // 10))))
        parts.append(_rand(rng, rng.integers(100, 3000)))
    return [np.concatenate(parts[:len(parts) // 2]), np.concatenate(parts[len(parts) // 2:])]


# slice_edges: what stands where against the first position p0 of a rank's slice
SLICE_EDGE_KINDS = ("sep_at_p0_minus_1", "sep_at_p0", "sep_at_p0_plus_1", "last_k_minus_1_straddle_p0")
SLICE_EDGE_OFFSET = {"sep_at_p0_minus_1": -1, "sep_at_p0": 0, "sep_at_p0_plus_1": 1, "last_k_minus_1_straddle_p0": 5}
SLICE_EDGE_N = 2400


def slice_edge_layout(G):
    """The variants of slice_edges for G shards: a list of {rank: kind}.  G - 1 ranks have a slice that starts inside the
    text; the four kinds are dealt out over them, in as many variants as that takes (4 at G = 2, 2 at G = 3, 1 at G = 8)."""
    ranks = list(range(1, G))
    per_variant = min(len(ranks), len(SLICE_EDGE_KINDS))
    out = []
    for i in range(0, len(SLICE_EDGE_KINDS), per_variant):
        kinds = SLICE_EDGE_KINDS[i:i + per_variant]
        out.append({ranks[j]: kind for j, kind in enumerate(kinds)})
    return out


def slice_edges(G, variant):
    """Records cut by the slice rule: the text has SLICE_EDGE_N symbols, so rank r's slice starts at
    p0 = r * (((SLICE_EDGE_N // G) >> 5) << 5), and for every (rank, kind) of the variant a separator stands at p0 - 1, at
    p0, at p0 + 1, or at p0 + 5 (the record's last k - 1 positions -- its special suffixes -- then lie on both sides of p0 for
    k = 12 and k = 32 alike).  The other separators fall where records of 33..400 bases put them.  Records are windows of
    one 2,000-base genome with a shared segment pasted into most of them and shared ends on some (the recipe of
    test_gpu_parity._adversarial), so that record ends meet inside nodes and special branches exist."""
    n = SLICE_EDGE_N
    per = ((n // G) >> 5) << 5
    want = sorted(per * r + SLICE_EDGE_OFFSET[kind] for r, kind in slice_edge_layout(G)[variant].items())
    rng = np.random.default_rng(1000 * G + variant)
    seps, at = [], 0                                      # `at`: first position of the record being cut
    for target in want + [n - 1]:
        while target - at > 400:                          # records of 150..400 bases up to the next fixed separator,
            L = int(rng.integers(150, 401))               # leaving at least 33 bases for the last of them
            if target - (at + L + 1) < 33:
                L = target - at - 1 - 33
            seps.append(at + L)
            at += L + 1
        assert 33 <= target - at <= 400, (G, variant, target, at)
        seps.append(target)
        at = target + 1
    genome = _rand(rng, 2000)
    base = _rand(rng, rng.integers(60, 200))
    recs, at = [], 0
    for s in seps:
        L = s - at
        p = int(rng.integers(0, len(genome) - L + 1))
        x = genome[p:p + L].copy()
        if rng.random() < 0.7:
            seg = base[:min(len(base), L)]
            q = int(rng.integers(0, L - len(seg) + 1))
            x[q:q + len(seg)] = seg
        if rng.random() < 0.4:
            x[-min(L, 40):] = base[:min(L, 40)]
        recs.append(x)
        at = s + 1
    assert at == n and 6 <= len(recs) <= 12, (G, variant, len(recs))
    return recs


class Case:
    def __init__(self, name, k, make, expect, worlds=WORLDS, entry=None, large_first=False, large_last=False, edges=None):
        self.name, self.k, self._make, self.expect, self.worlds, self.entry = name, k, make, expect, tuple(worlds), entry
        self.large_first, self.large_last = large_first, large_last          # a block above 2048 rows in shard 0 / G - 1
        self.edges = edges                                                    # slice_edges: {rank: kind}
        self._recs = None

    def records(self):
        if self._recs is None:
            self._recs = self._make()
        return self._recs

    @property
    def n(self):
        return int(sum(len(r) for r in self.records())) + len(self.records())


def _make_cases():
    cases = {}
    for name in sorted(outside_domain_cases()):
        for k in (12, 32):
            cases[f"{name}-k{k}"] = Case(f"{name}-k{k}", k, (lambda nm=name: outside_domain_cases()[nm]), "naive")
    for e in golden_manifest():
        if e["k"] in (12, 32) and (e["n"] < 10000 or (e["name"], e["k"]) in (("pan_4x20k", 12), ("reads_20000", 32))):
            nm = f"{e['name']}-k{e['k']}"
            cases[nm] = Case(nm, e["k"], (lambda en=e: golden_records(en)), "golden", entry=e)
    # 3 keys for 8 shards: the splitter targets of shards 1 and 2 round down to 0, so they start AND end at bin 0
    cases["fewer_keys_than_shards-k32"] = Case("fewer_keys_than_shards-k32", 32, (lambda: [_rand(np.random.default_rng(33), 33)]),
                                               "naive", worlds=(8,))
    cases["blocks_first_middle_last"] = Case("blocks_first_middle_last", 32, blocks_first_middle_last, "oracle",
                                             large_first=True, large_last=True)
    cases["deep_ties"] = Case("deep_ties", 32, deep_ties, "oracle", large_last=True)
    cases["periodic"] = Case("periodic", 32, periodic, "oracle")
    for G in WORLDS:
        for v, layout in enumerate(slice_edge_layout(G)):
            for k in (12, 32):
                nm = f"slice_edges_g{G}_{v}-k{k}"
                cases[nm] = Case(nm, k, (lambda g=G, vv=v: slice_edges(g, vv)), "oracle", worlds=(G,), edges=layout)
    return cases


CASES = _make_cases()
OUTSIDE = [nm for nm, c in CASES.items() if c.expect == "naive" and len(c.worlds) == 3]
FEWER_KEYS = "fewer_keys_than_shards-k32"
SMALL_GOLDENS = [nm for nm, c in CASES.items() if c.expect == "golden" and c.entry["n"] < 10000]
MIDSIZE_GOLDENS = [nm for nm, c in CASES.items() if c.expect == "golden" and c.entry["n"] >= 10000]
BLOCK_CASES = ["blocks_first_middle_last", "deep_ties"]
SLICE_EDGES = [nm for nm, c in CASES.items() if c.edges]


def case_worlds(names):
    """(case name, G) for every shard count a case runs at."""
    return [(nm, G) for nm in names for G in CASES[nm].worlds]


def sharded_launch_cases(world):
    """The cases of one launch of tests/test_sharded_edges_gpu.py, in the order the ranks take them: the collection with
    the large blocks first, last and in the middle of the small ones."""
    big = "blocks_first_middle_last"
    small = OUTSIDE + SMALL_GOLDENS + [nm for nm in SLICE_EDGES if CASES[nm].worlds == (world,)]
    return [big] + small[:len(small) // 2] + [big] + small[len(small) // 2:] + [big]


# ---- expected results --------------------------------------------------------------------------------------------

_EXPECTED = {}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def expected(name, oracle):
    """The expected result of a case, computed once per process: ("naive", row symbols) or ("oracle", words, '#' rows, '$'
    row); a golden case has it in the manifest."""
    c = CASES[name]
    if c.expect == "golden":
        return None
    if name not in _EXPECTED:
        sym = oracle.sym_from_codes(c.records())
        _EXPECTED[name] = oracle.naive_bwt(sym) if c.expect == "naive" else oracle.build_bwt(sym, c.k)
    return _EXPECTED[name] if c.expect == "naive" else _EXPECTED[name][:3]


def oracle_stats(name, oracle):
    """Counters of the oracle's build of an "oracle" case."""
    expected(name, oracle)
    return _EXPECTED[name][3]


def check_result(name, oracle, words, hrows, drow):
    """None when (words, '#' rows, '$' row) is the expected result of the case, else what differs."""
    c = CASES[name]
    if c.expect == "golden":
        sha = c.entry["sha256"]
        if _sha(words) != sha["bwt"]:
            return "BWT words differ from the reference's (sha256)"
        if _sha(hrows) != sha["hash"]:
            return "'#' rows differ from the reference's (sha256)"
        if _sha(np.array([drow], dtype=np.uint64)) != sha["dollar"]:
            return "'$' row differs from the reference's (sha256)"
        files = golden_outputs(c.entry)
        if files and not (np.array_equal(words, files[0]) and np.array_equal(hrows, files[1]) and drow == files[2]):
            return "result differs from the reference's output files"
        return None
    want = expected(name, oracle)
    if c.expect == "naive":
        if len(hrows) != len(c.records()) - 1 or (len(hrows) >= 2 and not bool((np.diff(hrows.astype(np.int64)) > 0).all())):
            return "'#' rows are not nrec - 1 ascending rows"
        got = oracle.unpack_bwt(words, c.n, hrows, drow)
        if not np.array_equal(got, want):
            return f"row symbols differ from the definition (first at row {int(np.flatnonzero(got != want)[0])})"
        return None
    if not np.array_equal(words, want[0]):
        return f"BWT words differ from the oracle's (first at word {int(np.flatnonzero(words != want[0])[0])})"
    if not np.array_equal(hrows, want[1]):
        return "'#' rows differ from the oracle's"
    if drow != want[2]:
        return f"'$' row {drow} differs from the oracle's {want[2]}"
    return None
