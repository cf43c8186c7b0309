"""Reference of the ONE alignment that include/debwt_hip.h documents for debwt_fm_extend and debwt_fm_extend_chain, written
out literally: H, E and F cell by cell over the allowed cells of a chain (a fixed band is the chain of one anchor), the end
cell as the largest H, then the smallest query index, then the smallest text position, and the walk back under the tie
rule -- in H the diagonal before E before F, stopping on the diagonal where H(i-1,t-1) <= 0; in E and F a gap is opened
rather than continued on a tie.  No GPU, no library."""
from fm_chain_ref import NEG, centres


def path_ref(q, text, rs, re, anchors, w, sc, info=None):
    """(score, qbeg, qend, tbeg, tend, edits, ops) of the documented alignment; ops: a list of BAM-coded ints
    (len << 4 | op, M 0, I 1, D 2), left to right.  q: the query as aligned (upper case); text: the whole text, so that
    tbeg and tend are global positions; [rs, re): the record's bases.  info (a dict, optional) receives what the path met:
    'ties': steps of the walk at which two sources reached the maximum; 'cross64': deletion steps taken at band index 64,
    i.e. entering E or H at band index 63 of the same row; 'end': the end cell (i, t); 'end_ties': the other cells that
    hold the largest H."""
    a, b, o, e = sc
    m, nb = len(q), 2 * w + 1
    cen = centres(anchors, m)
    rows = []                                               # row i: (text position of band index 0, H, E, F by band index)
    best, bi, bt, nbest = 0, 0, 0, 0
    for i in range(m):
        t0 = i + cen[i] - w
        H, E, F = [NEG] * nb, [NEG] * nb, [NEG] * nb
        if i:
            p0, Hp, _, Fp = rows[i - 1]
        for k in range(max(0, rs - t0), min(nb, re - t0)):
            t = t0 + k
            hl, el = (H[k - 1], E[k - 1]) if k else (NEG, NEG)
            hd = hu = fu = NEG
            if i:
                kd = t - 1 - p0
                if 0 <= kd < nb:
                    hd = Hp[kd]
                if 0 <= kd + 1 < nb:
                    hu, fu = Hp[kd + 1], Fp[kd + 1]
            ev = max(hl - o - e, el - e)
            fv = max(hu - o - e, fu - e)
            s = a if q[i] in "ACGT" and q[i] == text[t] else -b
            hv = max(0 + s, hd + s, ev, fv)
            H[k], E[k], F[k] = hv, ev, fv
            if hv > best:                                   # rows ascend, then text positions: the first one met stays
                best, bi, bt, nbest = hv, i, t, 1
            elif hv == best:
                nbest += 1
        rows.append((t0, H, E, F))
    if info is not None:
        info.update(ties=0, cross64=0, end=(bi, bt), end_ties=nbest - 1 if best else 0)
    if best == 0:
        return 0, 0, 0, 0, 0, 0, []

    def at(x, i, t):                                        # x: 1 H, 2 E, 3 F; -inf at a cell that is not allowed
        if i < 0:
            return NEG
        k = t - rows[i][0]
        return rows[i][x][k] if 0 <= k < nb else NEG

    i, t, state = bi, bt, 0                                 # state 0: in H, 1: in E (deletion), 2: in F (insertion)
    cols, edits, ties, cross = [], 0, 0, 0                  # cols: the op of every alignment column, last column first
    qbeg = tbeg = 0
    while True:
        assert rs <= t < re and 0 <= i < m and abs(t - i - cen[i]) <= w, (i, t)
        if state == 0:
            h, hd = at(1, i, t), at(1, i - 1, t - 1)
            s = a if q[i] in "ACGT" and q[i] == text[t] else -b
            dv, ev, fv = max(0, hd) + s, at(2, i, t), at(3, i, t)
            ties += (dv == h) + (ev == h) + (fv == h) >= 2
            if dv == h:
                cols.append(0)
                edits += s < 0
                qbeg, tbeg = i, t
                if hd <= 0:
                    break
                i, t = i - 1, t - 1
            elif ev == h:
                state = 1
            else:
                assert fv == h
                state = 2
        elif state == 1:
            cont, opened = at(2, i, t - 1) - e, at(1, i, t - 1) - o - e
            assert max(cont, opened) == at(2, i, t)
            ties += cont == opened
            cross += t - i - cen[i] + w == 64
            cols.append(2)
            edits += 1
            state = 1 if cont > opened else 0
            t -= 1
        else:
            cont, opened = at(3, i - 1, t) - e, at(1, i - 1, t) - o - e
            assert max(cont, opened) == at(3, i, t)
            ties += cont == opened
            cols.append(1)
            edits += 1
            state = 2 if cont > opened else 0
            i -= 1
    ops = []
    for op in reversed(cols):
        if ops and ops[-1][0] == op:
            ops[-1][1] += 1
        else:
            ops.append([op, 1])
    if info is not None:
        info.update(ties=int(ties), cross64=int(cross))
    return best, qbeg, bi + 1, tbeg, bt + 1, int(edits), [(n << 4) | op for op, n in ops]


def cigar_of(ops):
    return "".join(f"{x >> 4}{'MID'[x & 15]}" for x in ops)
