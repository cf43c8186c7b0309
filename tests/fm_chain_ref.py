"""References of the chain tests, written out literally from include/debwt_hip.h: chaining of one read's seeds
(chain_ref), the allowed cells and the DP of an extension along a chain (centres, chain_dp, chain_dp_rows), and the
reads with one-sided indels that a fixed band cannot follow (drift_reads).  No GPU, no library."""
import bisect

import numpy as np

NEG = -10 ** 9
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(p):
    return "".join(COMP.get(c, "N") for c in reversed(p.upper()))


def chain_ref(seeds, band=16, max_gap=5000, max_chains=8):
    """seeds: (strand, record, diag, qbeg, qend) -> [{score, strand, record, anchors: [(qbeg, diag)]}], best first"""
    S = sorted((st, rec, dg + qb, qb, qe, dg) for st, rec, dg, qb, qe in seeds)      # (strand, record, tbeg, qbeg, qend)
    n = len(S)
    ln = [s[4] - s[3] for s in S]
    tend = [s[5] + s[4] for s in S]
    f, pred = [0] * n, [-1] * n
    for j in range(n):
        top, who = None, -1
        for i in range(j):
            a, b = S[i], S[j]
            if (a[0], a[1]) != (b[0], b[1]):
                continue
            if not (a[3] < b[3] and a[4] < b[4] and a[2] < b[2] and tend[i] < tend[j]):
                continue
            if abs(b[5] - a[5]) > band or b[3] - a[4] > max_gap or b[2] - tend[i] > max_gap:
                continue
            v = f[i] + min(ln[j], b[4] - a[4], tend[j] - tend[i]) - abs(b[5] - a[5])
            if top is None or v >= top:                                             # the largest i of a tie
                top, who = v, i
        if top is not None and top >= ln[j]:                                        # no predecessor only when strictly better
            f[j], pred[j] = top, who
        else:
            f[j] = ln[j]
    used = [False] * n
    chains = []
    for e in sorted(range(n), key=lambda x: (-f[x], x)):
        if used[e]:
            continue
        walk, p = [], e
        while p >= 0 and not used[p]:
            walk.append(p)
            p = pred[p]
        for x in walk:
            used[x] = True
        first = S[walk[-1]]
        chains.append((-(f[e] - (f[p] if p >= 0 else 0)), first[0], first[1], first[5], first[3], len(chains), walk))
    chains.sort(key=lambda c: c[:6])
    return [{"score": -c[0], "strand": c[1], "record": c[2], "anchors": [(S[x][3], S[x][5]) for x in reversed(c[6])]}
            for c in chains[:max_chains]]


def centres(anchors, m):
    """c(i) of every query row: the diag of the last anchor with qbeg <= i, the first anchor's before it"""
    qs = [q for q, _ in anchors]
    return [anchors[max(bisect.bisect_right(qs, i) - 1, 0)][1] for i in range(m)]


def chain_dp(q, text, rs, re, anchors, w, sc):
    """the recurrence cell by cell over the allowed cells: (score, end row, end text position) -- the largest H, then
    the smallest row, then the smallest text position; q: the query as aligned (upper case)"""
    a, b, o, e = sc
    cen = centres(anchors, len(q))
    Hp, Fp = {}, {}
    best, bi, bt = 0, 0, 0
    for i in range(len(q)):
        H, F, E = {}, {}, {}
        for t in range(max(rs, i + cen[i] - w), min(re, i + cen[i] + w + 1)):
            ev = max(H.get(t - 1, NEG) - o - e, E.get(t - 1, NEG) - e)
            fv = max(Hp.get(t, NEG) - o - e, Fp.get(t, NEG) - e)
            s = a if q[i] in "ACGT" and q[i] == text[t] else -b
            hv = max(s, Hp.get(t - 1, NEG) + s, ev, fv)
            H[t], E[t], F[t] = hv, ev, fv
            if hv > best:
                best, bi, bt = hv, i, t
        Hp, Fp = H, F
    return best, bi, bt


def chain_dp_rows(qcodes, tcodes, rs, re, anchors, w, sc):
    """the same recurrence one row at a time in numpy (for a query too long for chain_dp): the score only.  E of a row is
    the running maximum of (H without its E term) - o - distance * e, which is the recurrence because o >= 0.
    qcodes: 0..3, 4 for a character that matches nothing; tcodes: the text's codes."""
    a, b, o, e = sc
    m, nb = len(qcodes), 2 * w + 1
    cen = centres(anchors, m)
    k = np.arange(nb, dtype=np.int64)
    big = np.int64(NEG)
    Hp = np.full(nb + 2 * w + 2, big)                       # the row before, padded by w + 1 on each side
    Fp = Hp.copy()
    best = 0
    tc = np.asarray(tcodes, dtype=np.int64)
    for i in range(m):
        d = cen[i] - cen[i - 1] if i else 0
        t = i + cen[i] - w + k
        ok = (t >= rs) & (t < re)
        if not ok.any():
            Hp[:] = big
            Fp[:] = big
            continue
        s = np.where(ok & (tc[np.clip(t, 0, len(tc) - 1)] == qcodes[i]), a, -b)
        hd = Hp[w + 1 + d:w + 1 + d + nb]                   # band index k + d of the row before
        hu = Hp[w + 2 + d:w + 2 + d + nb]
        fu = Fp[w + 2 + d:w + 2 + d + nb]
        F = np.maximum(hu - o - e, fu - e)
        h0 = np.maximum(hd, 0) + s
        x = np.where(ok, np.maximum(h0, F) + k * e, big)
        run = np.maximum.accumulate(x)
        E = np.concatenate(([big], run[:-1])) - o - k * e
        H = np.where(ok, np.maximum(np.maximum(h0, E), F), big)
        F = np.where(ok, F, big)
        best = max(best, int(H.max()))
        Hp[:] = big
        Fp[:] = big
        Hp[w + 1:w + 1 + nb] = np.maximum(H, big)
        Fp[w + 1:w + 1 + nb] = np.maximum(F, big)
    return best


def drift_reads(strs, seed, count=40):
    """reads of 1500..3000 bases cut from the records `strs`, every second one given as its reverse complement, each with
    4..8 indels of 10..40 bases, all insertions or all deletions, edits at least 60 bases apart, total drift >= 100:
    [(read as given, strand, record, start in the record)]"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        rec = int(rng.integers(0, len(strs)))
        L = int(rng.integers(1500, 3001))
        a = int(rng.integers(0, len(strs[rec]) - L - 400))
        nev = int(rng.integers(4, 9))
        sizes = [int(x) for x in rng.integers(10, 41, nev)]
        if sum(sizes) < 100:
            continue
        ins = bool(rng.integers(0, 2))
        # edit positions in the segment, at least 100 apart and away from the ends (60 after a deletion of up to 40)
        slots = sorted(int(x) for x in rng.choice(np.arange(1, L // 100 - 1), size=nev, replace=False))
        parts, cur = [], 0
        seg = strs[rec][a:a + L + 400]
        for slot, n in zip(slots, sizes):
            c = 100 * slot
            parts.append(seg[cur:c])
            if ins:
                parts.append("".join("ACGT"[int(x)] for x in rng.integers(0, 4, n)))
                cur = c
            else:
                cur = c + n
        parts.append(seg[cur:L])
        read = "".join(parts)
        strand = len(out) % 2
        out.append((revcomp(read) if strand else read, strand, rec, a))
    return out
