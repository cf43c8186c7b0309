"""Definitions 7 and 8 of include/debwt_hip.h, the insertion vote and the consensus, written out literally: a loop over
ops and columns, a dict of counts.  No GPU, no library.  An alignment is (pattern, tbeg, qbeg, strand) with a list of
BAM-coded ops (len << 4 | op, M 0, I 1, D 2)."""
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
SLOT = {"A": 0, "C": 1, "G": 2, "T": 3}
DEL, INS, OTHER, NO_CALL, INS_BIT = 4, 5, 6, 5, 0x10


class Invalid(Exception):
    """what the library answers with DEBWT_EINVAL"""


def query(p, strand):
    """Q: the pattern or its reverse complement, upper case, every non-base an 'N'"""
    q = "".join(c if c in "ACGT" else "N" for c in p.upper())
    return q if strand == 0 else "".join(COMP.get(c, "N") for c in reversed(q))


def text_of(strs):
    """the text (records joined by '#', '$' at the end) and the first position of every record"""
    starts, o = [], 0
    for s in strs:
        starts.append(o)
        o += len(s) + 1
    return "#".join(strs) + "$", starts


def check(patterns, alns, cigars, n, window):
    wbeg, wend = window
    if wend <= wbeg or wend > n:
        raise Invalid("window")
    for (p, tbeg, qbeg, strand), ops in zip(alns, cigars):
        if p >= len(patterns) or strand > 1:
            raise Invalid("pattern or strand")
        q = t = 0
        for k, x in enumerate(ops):
            kind, ln = x & 15, x >> 4
            if kind > 2 or ln == 0 or ((k == 0 or k == len(ops) - 1) and kind != 0):
                raise Invalid("op")
            q += ln if kind != 2 else 0
            t += ln if kind != 1 else 0
        if qbeg + q > len(patterns[p]) or tbeg + t > n:
            raise Invalid("past the end")


def events(patterns, alns, cigars):
    """every event of definition 7 as (t, slot), unclipped; and the insertions as (t, aln, qpos, len)"""
    ev, ins = [], []
    for g, ((p, tbeg, qbeg, strand), ops) in enumerate(zip(alns, cigars)):
        Q = query(patterns[p], strand)
        i, t = qbeg, tbeg
        for x in ops:
            kind, ln = x & 15, x >> 4
            if kind == 0:
                for _ in range(ln):
                    ev.append((t, SLOT.get(Q[i], OTHER)))
                    i += 1
                    t += 1
            elif kind == 2:
                for _ in range(ln):
                    ev.append((t, DEL))
                    t += 1
            else:
                ev.append((t - 1, INS))
                ins.append((t - 1, g, i, ln))
                i += ln
    return ev, ins


def pileup(patterns, alns, cigars, n, window, table=None):
    """{(t, slot): count} over the window; table: a dict to add to (DEBWT_FM_PILE_ADD)"""
    check(patterns, alns, cigars, n, window)
    counts = {} if table is None else table
    for t, slot in events(patterns, alns, cigars)[0]:
        if window[0] <= t < window[1]:
            counts[(t, slot)] = counts.get((t, slot), 0) + 1
    return counts


def dense(counts, window):
    """the dict as rows of 8 counts, one per position of the window"""
    return [[counts.get((t, s), 0) for s in range(8)] for t in range(window[0], window[1])]


def call(counts, text, window, min_depth=4, min_permille=600):
    """(calls, ref, variants) of definition 8; a variant is (t, depth, count, ins, ref, call)"""
    calls, refs, variants = [], [], []
    for t in range(window[0], window[1]):
        c = [counts.get((t, s), 0) for s in range(8)]
        ref = SLOT.get(text[t], 4)
        d = sum(c[:5])
        top = max(c[:5])
        tied = [s for s in range(5) if c[s] == top]
        best = ref if ref in tied and ref != 4 else tied[0]
        called = ref != 4 and d >= min_depth and c[best] * 1000 >= min_permille * d
        cb = best if called else NO_CALL
        if called and c[INS] * 1000 >= min_permille * d:
            cb |= INS_BIT
        calls.append(cb)
        refs.append(ref)
        if called and (best != ref or cb & INS_BIT):
            variants.append((t, d, c[best], c[INS], ref, cb))
    return calls, refs, variants


def insertions(patterns, alns, cigars, positions):
    """the events (t, aln, qpos, len) anchored at a listed position, ordered by (t, aln, qpos)"""
    want = set(positions)
    return sorted(e for e in events(patterns, alns, cigars)[1] if e[0] in want)


def vote(patterns, alns, evs):
    """(string, support) of the events of one position: the most frequent string, then the shorter, then the smaller"""
    tally = {}
    for _, g, qpos, ln in evs:
        p, _, _, strand = alns[g]
        s = query(patterns[p], strand)[qpos:qpos + ln]
        tally[s] = tally.get(s, 0) + 1
    if not tally:
        return "", 0
    s = min(tally, key=lambda w: (-tally[w], len(w), w))
    return s, tally[s]


def consensus(text, starts, calls, window, voted, min_permille=600):
    """per record the consensus inside the window; voted: {t: (string, support, depth)}"""
    out = []
    n = len(text)
    for r, rs in enumerate(starts):
        re = (starts[r + 1] if r + 1 < len(starts) else n) - 1
        s = []
        for t in range(max(rs, window[0]), min(re, window[1])):
            c = calls[t - window[0]]
            b = c & 15
            if b < 4:
                s.append("ACGT"[b])
            elif b == NO_CALL:
                s.append(text[t].lower())
            if c & INS_BIT and t in voted and voted[t][1] * 1000 >= min_permille * voted[t][2]:
                s.append(voted[t][0])
        out.append("".join(s))
    return out


def run(patterns, alns, cigars, strs, window=None, min_depth=4, min_permille=600):
    """the whole pipeline on record strings: (dense table, calls, variants, voted {t: (string, support, depth)}, consensus)"""
    text, starts = text_of(strs)
    window = window or (0, len(text))
    counts = pileup(patterns, alns, cigars, len(text), window)
    calls, refs, variants = call(counts, text, window, min_depth, min_permille)
    flagged = [v for v in variants if v[5] & INS_BIT]
    evs = insertions(patterns, alns, cigars, [v[0] for v in flagged])
    voted = {}
    for v in flagged:
        s, sup = vote(patterns, alns, [e for e in evs if e[0] == v[0]])
        voted[v[0]] = (s, sup, v[1])
    return dense(counts, window), calls, variants, voted, consensus(text, starts, calls, window, voted, min_permille)
