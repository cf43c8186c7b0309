"""The compacted de Bruijn graph on the GPU (debwt_fm_cdbg; EsaResult.cdbg) against Definition 13 as cdbg_ref.py writes
it out.  Everything is compared exactly: unitig records, seq bytes, edges, sizes and the counting fields of the statistics,
on every geometry case, the seeded read set with the library's own profile and spectrum as second witnesses, a long chain
and a long cycle with the bound that pins the ranking to logarithmic rounds, a small pan-genome, capped builds and the
protocol."""
import ctypes
import functools
import math

import numpy as np
import pytest

import cdbg_ref as CR
import esa_ref as ER
import fm_definition as F
import repeat_ref as RR
from test_fm_cdbg_ref import chain_record, cycle_record, pan_genome
from test_fm_esa_gpu import index_of

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, ERANGE = -1, -4, -5
CASES = F.geometry_cases()
KS = (1, 2, 3, 5, 8)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


@functools.lru_cache(maxsize=None)
def esa_of(which):
    if which == "chain":
        return ER.Esa([chain_record()])
    if which == "cycle":
        return ER.Esa([cycle_record()])
    if which == "pan":
        return ER.Esa(pan_genome())
    return ER.of_read_set()


def check(x, e, E, k, max_lcp=0):
    """one call against the reference; returns (the library's answer, the reference, the statistics)"""
    want = CR.from_esa(E, k, max_lcp)
    got = e.cdbg(k)
    assert got.unitigs.dtype == CR.UNITIG_DTYPE and got.edges.dtype == CR.EDGE_DTYPE and got.seq.dtype == np.uint8
    assert np.array_equal(got.unitigs, want.unitigs), k
    assert np.array_equal(got.seq, want.seq) and np.array_equal(got.edges, want.edges), k
    assert got.strings() == want.strings()
    st = x.cdbg_stats()
    assert {name: st[name] for name in CR.COUNTING} == want.counts, k
    assert st["jump_steps"] <= st["nodes"] * st["jump_rounds"] and st["jump_steps"] <= st["jump_wave_steps"]
    assert (st["jump_rounds"] == 0) == (st["links"] + st["circular"] == 0)
    assert st["scratch_bytes"] > 0 and st["ms_wall"] > 0
    return got, want, st


def round_bound(st):
    return 2 * math.ceil(math.log2(st["longest_nodes"])) + 4


# ---- every geometry case ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_geometry_cases(api, name):
    E = ER.of_case(name)
    x = index_of(api, CASES[name], 32)
    e = x.esa(sa=True, da=True)
    for k in KS:
        got, want, st = check(x, e, E, k)
        if name in ("ones_600", "short_1to3_x500") and k >= 5:
            assert (len(got.unitigs), len(got.seq), len(got.edges), st["nodes"]) == (0, 0, 0, 0)
        if name in ("all_T_x3", "homopolymer_only_one_record") and k == 8:
            assert len(got.unitigs) == 1 and got.edges.tolist() == [(0, 0)] and got.unitigs["kmer_count"][0] >= 380
    x.close()


# ---- the seeded read set ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [15, 21, 31])
def test_read_set(api, k):
    E = esa_of("reads")
    x = index_of(api, E.records, 4)
    e = x.esa(sa=True, da=True)
    got, want, st = check(x, e, E, k)
    prof = e.profile(k + 1)
    nodes = int(got.unitigs["nodes"].astype(np.int64).sum())
    assert nodes == prof[k - 1] == st["nodes"]                                           # fact 1
    assert nodes - len(got.unitigs) + len(got.edges) == prof[k] == st["edge_strings"]   # fact 2
    assert int(got.unitigs["kmer_count"].sum()) == x.spectrum(k, strands="forward").total   # fact 3
    assert st["circular"] == want.counts["circular"] and len(got.unitigs) > 100
    x.close()


# ---- the bounds that pin the ranking --------------------------------------------------------------------------------------

def test_long_chain(api):
    """One record of 20,000 random bases at k = 16: one unitig of 19,985 nodes.  A linear walk would need 19,985 rounds."""
    E = esa_of("chain")
    x = index_of(api, E.records, 32)
    e = x.esa(sa=True, da=True)
    got, want, st = check(x, e, E, 16)
    assert got.unitigs["nodes"].tolist() == [19985] and len(got.edges) == 0 and st["longest_nodes"] == 19985
    print(f"jump_rounds {st['jump_rounds']}, bound {round_bound(st)}, jump_steps {st['jump_steps']}, nodes {st['nodes']}")
    assert st["jump_rounds"] <= round_bound(st) and st["jump_steps"] <= st["nodes"] * st["jump_rounds"]
    got, want, st = check(x, e, E, 12)
    assert (len(got.unitigs), len(got.edges), st["longest_nodes"]) == (22, 28, 4493)
    assert st["jump_rounds"] <= round_bound(st)
    x.close()


def test_long_cycle(api):
    """A 5,000-base unit three times over at k = 16: one circular unitig of 5,000 nodes from its lowest k-mer."""
    E = esa_of("cycle")
    x = index_of(api, E.records, 32)
    e = x.esa(sa=True, da=True)
    got, want, st = check(x, e, E, 16)
    assert got.unitigs["nodes"].tolist() == [5000] and got.unitigs["kmer_count"].tolist() == [14985]
    assert got.unitigs["flags"].tolist() == [CR.CIRCULAR] and got.edges.tolist() == [(0, 0)] and st["circular"] == 1
    s = F.strings(E.records)[0]
    assert got.strings()[0][:16] == min(s[i:i + 16] for i in range(5000))
    print(f"jump_rounds {st['jump_rounds']}, bound {round_bound(st)}, jump_steps {st['jump_steps']}, nodes {st['nodes']}")
    assert st["jump_rounds"] <= round_bound(st) and st["jump_steps"] <= st["nodes"] * st["jump_rounds"]
    x.close()


def test_pan_genome(api):
    """four copies of a 5,000-base genome with 1 % substitutions at k = 21: bubbles, shared heads and tails"""
    E = esa_of("pan")
    x = index_of(api, E.records, 32)
    e = x.esa(sa=True, da=True)
    got, want, st = check(x, e, E, 21)
    assert (len(got.unitigs), len(got.edges), st["nodes"]) == (487, 649, 9026)
    x.close()


# ---- caps ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,k", [("dup_40x20", 8), ("homopolymer_only_one_record", 5), ("n768", 3)])
def test_caps(api, name, k):
    E = ER.of_case(name)
    x = index_of(api, CASES[name], 32)
    e = x.esa(sa=True, da=True)
    full, _, _ = check(x, e, E, k)
    e = x.esa(max_lcp=k + 1, sa=True, da=True)
    capped, _, _ = check(x, e, E, k, max_lcp=k + 1)
    assert capped.unitigs.tobytes() == full.unitigs.tobytes() and capped.seq.tobytes() == full.seq.tobytes()
    assert capped.edges.tobytes() == full.edges.tobytes()
    e = x.esa(max_lcp=k, sa=True, da=True)
    assert code_of(api, e.cdbg, k) == EINVAL
    assert len(e.cdbg(k - 1).unitigs) == len(CR.from_esa(E, k - 1).unitigs)
    x.close()


# ---- protocol -----------------------------------------------------------------------------------------------------------

def code_of(api, fn, *args, **kw):
    with pytest.raises(api.DebwtError) as err:
        fn(*args, **kw)
    return err.value.code


def raw(x, k, un, seq, ed, caps, flags=0, sizes=True):
    from debwt_amd import _lib
    sz = _lib.DebwtFmCdbgSizes(11, 12, 13)
    p = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in (un, seq, ed)]
    rc = x._L.debwt_fm_cdbg(x._h, k, flags, p[0], caps[0], p[1], caps[1], p[2], caps[2], ctypes.byref(sz) if sizes else None)
    return rc, (sz.unitigs, sz.seq_bytes, sz.edges)


def test_protocol(api):
    name, k = "n768", 3
    E = ER.of_case(name)
    want = CR.from_esa(E, k)
    U, B, M = want.sizes()
    assert U > 3 and M > 3
    x = index_of(api, CASES[name], 4)
    untouched = (11, 12, 13)
    assert code_of(api, api.EsaResult(x).cdbg, k) == ESTATE                      # no build
    assert raw(x, k, None, None, None, (0, 0, 0)) == (ESTATE, untouched)
    for kw in ({"sa": True}, {"da": True}, {}):                                  # a build without da, without sa, without both
        e = x.esa(**kw)
        assert code_of(api, e.cdbg, k) == ESTATE and raw(x, k, None, None, None, (0, 0, 0)) == (ESTATE, untouched)
    e = x.esa(sa=True, da=True)
    lcp0, sa0, da0, b0 = e.lcp(), e.sa(), e.da(), x.info()["device_bytes"]
    rep0 = e.repeats(min_len=2)
    un, seq, ed = np.zeros(U + 1, dtype=CR.UNITIG_DTYPE), np.zeros(B + 1, dtype=np.uint8), np.zeros(M + 1, dtype=CR.EDGE_DTYPE)
    assert raw(x, 0, None, None, None, (0, 0, 0)) == (EINVAL, untouched)         # k = 0
    assert raw(x, k, None, None, None, (0, 0, 0), flags=1) == (EINVAL, untouched)
    assert raw(x, k, None, None, None, (0, 0, 0), sizes=False)[0] == EINVAL
    for caps in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):                               # a NULL array with capacity > 0
        assert raw(x, k, None, None, None, caps) == (EINVAL, untouched)
    assert raw(x, k, None, None, None, (0, 0, 0)) == (ERANGE, (U, B, M))         # the sizing call
    for caps in ((U - 1, B, M), (U, B - 1, M), (U, B, M - 1)):                   # each capacity one short
        assert raw(x, k, un, seq, ed, caps) == (ERANGE, (U, B, M)), caps
        assert not un.view(np.uint8).any() and not seq.any() and not ed.view(np.uint8).any()
    assert raw(x, k, un, seq, ed, (U, B, M)) == (0, (U, B, M))
    assert np.array_equal(un[:U], want.unitigs) and np.array_equal(seq[:B], want.seq) and np.array_equal(ed[:M], want.edges)
    assert not un[U:].view(np.uint8).any() and not seq[B:].any() and not ed[M:].view(np.uint8).any()
    assert raw(x, k, un, seq, ed, (U + 1, B + 1, M + 1)) == (0, (U, B, M))
    assert raw(x, 2000, None, None, None, (0, 0, 0)) == (0, (0, 0, 0))            # every record is shorter: all sizes 0
    # the kept arrays are as they were, and the repeats answer the same
    assert np.array_equal(e.lcp(), lcp0) and np.array_equal(e.sa(), sa0) and np.array_equal(e.da(), da0)
    assert x.info()["device_bytes"] == b0
    assert np.array_equal(e.repeats(min_len=2), rep0) and np.array_equal(rep0, RR.repeats(E, min_len=2))
    e.release()
    assert code_of(api, e.cdbg, k) == ESTATE
    x.close()
