"""Chaining of one read's seeds (debwt_fm_chain_seeds): pure host code, driven on hand-made and random seeds without a
GPU, against the definition of include/debwt_hip.h written out literally (fm_chain_ref.chain_ref).  Seeds are (strand,
record, diag, qbeg, qend); a chain is (score, strand, record, anchors as (qbeg, diag))."""
import ctypes

import numpy as np
import pytest

from fm_chain_ref import chain_ref


@pytest.fixture(scope="module")
def chain():
    from debwt_amd import api
    return api.chain_seeds


def colinear_run(rng, strand, rec, diag, q, steps, gaps, ln=20):
    """seeds of length ln, one after the other: diagonal steps `steps`, query gaps `gaps` between consecutive seeds"""
    out = [(strand, rec, diag, q, q + ln)]
    for st, g in zip(steps, gaps):
        q = q + ln + g
        diag += st
        out.append((strand, rec, diag, q, q + ln))
    return out


def random_seeds(rng, n, band, max_gap):
    seeds = []
    while len(seeds) < n:
        kind = int(rng.integers(0, 6))
        st, rec = int(rng.integers(0, 2)), int(rng.integers(0, 3))
        diag, q = int(rng.integers(-50, 4000)), int(rng.integers(0, 400))
        if kind == 0:                                       # steps of exactly band and band + 1, both signs
            steps = [int(x) for x in rng.choice([band, -band, band + 1, -band - 1, 0, 1, -1], size=4)]
            seeds += colinear_run(rng, st, rec, diag, q, steps, [int(x) for x in rng.integers(0, 30, 4)])
        elif kind == 1:                                     # gaps of exactly max_gap and max_gap + 1, in the read or the text
            for g in (max_gap, max_gap + 1):
                seeds += colinear_run(rng, st, rec, diag, q, [0, int(rng.integers(-3, 4))], [g, 5])
                diag += 7 * max_gap
            qb = q + 20 + max_gap - min(band, max_gap)    # the text gap is max_gap, the read's is shorter
            seeds += [(st, rec, diag, q, q + 20), (st, rec, diag + min(band, max_gap), qb, qb + 25)]
        elif kind == 2:                                     # overlapping and nested seeds around one diagonal
            for _ in range(4):
                a = q + int(rng.integers(0, 30))
                seeds.append((st, rec, diag + int(rng.integers(-2, 3)), a, a + int(rng.integers(1, 40))))
        elif kind == 3:                                     # two equal runs side by side: equal f, equal scores
            run = colinear_run(rng, st, rec, diag, q, [1, 0], [3, 3])
            seeds += run + [(s, r, d + 5000, a, b) for s, r, d, a, b in run]
        else:                                               # noise
            ln = int(rng.integers(1, 60))
            seeds.append((st, rec, diag, q, q + ln))
    return seeds[:n] if n < 4 else seeds


@pytest.mark.parametrize("band,max_gap", [(16, 5000), (0, 50), (63, 300), (5, 0)])
def test_random_sets_against_definition(chain, band, max_gap):
    rng = np.random.default_rng(1000 * band + max_gap)
    sizes = [0, 1, 2, 2, 3, 10, 40, 120, 300]
    for n in sizes:
        seeds = random_seeds(rng, n, band, max_gap)
        for mc in (1, 8, len(seeds) + 5):
            want = chain_ref(seeds, band, max_gap, mc)
            got = chain(seeds, band=band, max_gap=max_gap, max_chains=mc)
            assert got == want, (n, mc)
        full = chain(seeds, band=band, max_gap=max_gap, max_chains=len(seeds) + 5)
        assert sum(len(c["anchors"]) for c in full) == len(seeds)           # every seed ends up in exactly one chain
        for c in full:
            qs = [q for q, _ in c["anchors"]]
            ds = [d for _, d in c["anchors"]]
            assert all(x < y for x, y in zip(qs, qs[1:])) and all(abs(x - y) <= band for x, y in zip(ds, ds[1:]))
        # input order does not matter
        perm = [seeds[int(x)] for x in rng.permutation(len(seeds))]
        assert chain(perm, band=band, max_gap=max_gap, max_chains=8) == chain(seeds, band=band, max_gap=max_gap, max_chains=8)
    assert chain([(0, 0, 5, 1, 9)], max_chains=0) == []


def test_hand_made_chains(chain):
    # three seeds along one alignment with a 20-base deletion and a 5-base insertion: one chain, all three anchors
    seeds = [(0, 1, 1000, 0, 50), (0, 1, 1020, 50, 120), (0, 1, 1015, 125, 200)]
    c = chain(seeds, band=20)
    assert c == [{"score": 50 + (70 - 20) + (75 - 5), "strand": 0, "record": 1, "anchors": [(0, 1000), (50, 1020), (125, 1015)]}]
    # the same with a band of 19: the first step does not fit, two chains, the heavier one first
    c = chain(seeds, band=19)
    assert [(x["score"], x["anchors"]) for x in c] == [(70 + 70, [(50, 1020), (125, 1015)]), (50, [(0, 1000)])]
    # overlapping seeds count the overlap once: gain = new query (and text) bases only
    c = chain([(1, 0, 70, 10, 40), (1, 0, 70, 30, 60)])
    assert c == [{"score": 30 + 20, "strand": 1, "record": 0, "anchors": [(10, 70), (30, 70)]}]
    # strands and records never mix; equal scores order by (strand, record, first diag, first qbeg)
    seeds = [(1, 0, 10, 0, 20), (0, 1, 500, 0, 20), (0, 1, 100, 30, 50), (0, 0, 900, 0, 20), (0, 1, 100, 5, 25)]
    c = chain(seeds, band=16, max_gap=3)
    assert [(x["strand"], x["record"], x["anchors"][0]) for x in c] == [
        (0, 0, (0, 900)), (0, 1, (5, 100)), (0, 1, (30, 100)), (0, 1, (0, 500)), (1, 0, (0, 10))]
    # a seed that two later seeds would like as their predecessor goes to the better chain; the other one starts at
    # its own seed and scores what it adds
    seeds = [(0, 0, 0, 0, 30), (0, 0, 2, 40, 100), (0, 0, -3, 40, 60)]
    c = chain(seeds)
    assert [(x["score"], x["anchors"]) for x in c] == [(30 + 60 - 2, [(0, 0), (40, 2)]), (20 - 3, [(40, -3)])]


def test_early_break_keeps_a_long_seed(chain):
    # the inner loop may stop once tbeg_j - tbeg_i exceeds max_gap + the longest seed: a seed of 3000 bases whose end
    # lies exactly max_gap before the next one starts 3000 + max_gap before it, with 40 short seeds of other diagonals
    # sorted between the two
    max_gap = 100
    seeds = [(0, 0, 0, 0, 3000), (0, 0, 0, 3000 + max_gap, 3150)]
    seeds += [(0, 0, 2000 - 30 * x, 400 + 30 * x, 410 + 30 * x) for x in range(40)]
    got = chain(seeds, band=16, max_gap=max_gap, max_chains=1)
    assert got == chain_ref(seeds, 16, max_gap, 1)
    assert got[0]["anchors"] == [(0, 0), (3100, 0)] and got[0]["score"] == 3000 + 50
    seeds[1] = (0, 0, 0, 3001 + max_gap, 3150)               # one base further: no longer a predecessor
    got = chain(seeds, band=16, max_gap=max_gap, max_chains=1)
    assert got == chain_ref(seeds, 16, max_gap, 1) and got[0]["anchors"] == [(0, 0)]


def test_errors_and_capacity_protocol(chain):
    from debwt_amd import _lib, api
    for seeds, kw in (([(0, 0, 5, 10, 10)], {}), ([(0, 0, 5, 10, 9)], {}), ([(0, 0, 5, 1, 9)], dict(band=64))):
        with pytest.raises(api.DebwtError) as e:
            chain(seeds, **kw)
        assert e.value.code == -1
    L = _lib.lib()
    seeds = [(0, 0, 0, 0, 30), (0, 0, 2, 40, 100), (0, 0, 900, 40, 60)]
    sa = (_lib.DebwtFmSeed * 3)()
    for k, (st, rec, dg, qb, qe) in enumerate(seeds):
        sa[k].strand, sa[k].record, sa[k].diag, sa[k].qbeg, sa[k].qend = st, rec, dg, qb, qe
    ch = (_lib.DebwtFmChain * 4)()
    an = (_lib.DebwtFmAnchor * 4)()
    need = ctypes.c_uint64(99)
    assert L.debwt_fm_chain_seeds(sa, 3, 16, 5000, 4, ch, an, 2, ctypes.byref(need)) == -5   # DEBWT_ERANGE
    assert need.value == 3 and (ch[0].n_anchors, ch[0].first_anchor, ch[1].n_anchors, ch[1].first_anchor) == (2, 0, 1, 2)
    assert L.debwt_fm_chain_seeds(sa, 3, 16, 5000, 1, ch, an, 2, ctypes.byref(need)) == 1 and need.value == 2
    assert [(an[x].qbeg, an[x].diag) for x in range(2)] == [(0, 0), (40, 2)]
    assert L.debwt_fm_chain_seeds(sa, 3, 16, 5000, 4, ch, an, 3, ctypes.byref(need)) == 2 and need.value == 3
    assert (an[2].qbeg, an[2].diag, ch[1].score) == (40, 900, 20)
    assert L.debwt_fm_chain_seeds(sa, 0, 16, 5000, 4, ch, an, 0, ctypes.byref(need)) == 0 and need.value == 0
