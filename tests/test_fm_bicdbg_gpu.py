"""The compacted de Bruijn graph over both strands on the GPU (debwt_fm_cdbg_both; EsaResult.cdbg(k, strands="both"))
against Definition 14 as bicdbg_ref.py writes it out.  Everything is compared exactly: unitig records, seq bytes, edges,
sizes and the counting fields of the statistics, on every geometry case, a seeded read set with every second read
reverse-complemented (the library's own spectrum as second witness), an index of the doubled collection folded as another
witness wherever the reference reports no hairpin, a long chain and a long cycle with the bound that pins the ranking to
logarithmic rounds, the hairpin and dedup collections, capped builds, the protocol, and the forward call left as it was."""
import ctypes
import functools
import math

import numpy as np
import pytest

import bicdbg_ref as BR
import cdbg_ref as CR
import esa_ref as ER
import fm_definition as F
from test_fm_bicdbg_ref import FOLD_PAN, FOLD_READS, mixed_reads
from test_fm_cdbg_ref import chain_record, codes, cycle_record, pan_genome
from test_fm_esa_gpu import index_of

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, ERANGE = -1, -4, -5
CASES = F.geometry_cases()
KS = (1, 3, 5, 7)


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
    if which == "cycle2":
        return ER.Esa([cycle_record(), BR.rc_codes(cycle_record())])
    if which == "pan":
        return ER.Esa(pan_genome())
    return ER.Esa(mixed_reads())


@functools.lru_cache(maxsize=None)
def want_of(which, k):
    return BR.from_esa(esa_of(which), k)


def check(x, e, want, k):
    """one call against the reference; returns (the library's answer, the statistics)"""
    got = e.cdbg(k, strands="both")
    assert got.strands == "both"
    assert got.unitigs.dtype == CR.UNITIG_DTYPE and got.edges.dtype == CR.EDGE_DTYPE and got.seq.dtype == np.uint8
    assert np.array_equal(got.unitigs, want.unitigs), k
    assert np.array_equal(got.seq, want.seq) and np.array_equal(got.edges, want.edges), k
    assert got.strings() == want.strings()
    st = x.cdbg_both_stats()
    assert {name: st[name] for name in BR.COUNTING} == want.counts, k
    assert st["jump_steps"] <= (2 * st["present"] - st["mated"]) * st["jump_rounds"] and st["jump_steps"] <= st["jump_wave_steps"]
    assert (st["jump_rounds"] == 0) == (st["links"] + st["circular"] == 0)
    assert st["mate_steps"] <= k * st["present"] and (st["mate_steps"] >= st["present"] or not st["present"])
    assert st["edges"] <= st["edge_keys"] <= 2 * st["edges"] or not len(got.unitigs)
    assert st["scratch_bytes"] > 0 and st["ms_wall"] > 0
    return got, st


def round_bound(st):
    return 2 * math.ceil(math.log2(st["longest_nodes"])) + 4


# ---- every geometry case ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_geometry_cases(api, name):
    E = ER.of_case(name)
    x = index_of(api, CASES[name], 32)
    e = x.esa(sa=True, da=True)
    for k in KS:
        got, st = check(x, e, BR.from_esa(E, k), k)
        if name in ("ones_600", "short_1to3_x500") and k >= 5:
            assert (len(got.unitigs), len(got.seq), len(got.edges), st["nodes"]) == (0, 0, 0, 0)
    x.close()


# ---- the seeded read set ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [15, 21, 31])
def test_read_set(api, k):
    E = esa_of("reads")
    x = index_of(api, E.records, 4)
    e = x.esa(sa=True, da=True)
    got, st = check(x, e, want_of("reads", k), k)
    nodes = int(got.unitigs["nodes"].astype(np.int64).sum())
    assert nodes == x.spectrum(k, strands="both").distinct == st["nodes"]                    # fact 1
    assert 2 * (nodes - len(got.unitigs)) + len(got.edges) == st["edge_strings"]            # fact 2
    assert int(got.unitigs["kmer_count"].sum()) == x.spectrum(k, strands="forward").total   # fact 3
    assert 0 < st["mated"] < st["present"] and len(got.unitigs) > 100
    first = [s[:k] for s in got.strings()]
    present = BR.kmers_of(F.strings(E.records), k)
    assert any(w not in present for w in first) and any(w in present for w in first)        # some first nodes are absent from S
    x.close()


# ---- the doubled index as second witness ----------------------------------------------------------------------------------

@pytest.mark.parametrize("which,ks", [("reads", FOLD_READS), ("pan", FOLD_PAN)])
def test_doubled_index(api, which, ks):
    E = esa_of(which)
    x = index_of(api, E.records, 4)
    xd = index_of(api, BR.doubled(E.records), 4)
    e, ed = x.esa(sa=True, da=True), xd.esa(sa=True, da=True)
    strs = F.strings(E.records)
    for k in ks:
        assert want_of(which, k).counts["hairpins"] == 0
        got = e.cdbg(k, strands="both")
        assert x.cdbg_both_stats()["hairpins"] == 0
        assert BR.fold(ed.cdbg(k), k, BR.kmers_of(strs, k)) == BR.folded(got), k
    x.close()
    xd.close()


# ---- the bounds that pin the ranking --------------------------------------------------------------------------------------

def test_long_chain(api):
    """One record of 20,000 random bases at k = 15: one unitig of 19,986 nodes, and its mirror of as many ids."""
    E = esa_of("chain")
    x = index_of(api, E.records, 32)
    e = x.esa(sa=True, da=True)
    got, st = check(x, e, want_of("chain", 15), 15)
    assert got.unitigs["nodes"].tolist() == [19986] and len(got.edges) == 0 and st["longest_nodes"] == 19986
    print(f"jump_rounds {st['jump_rounds']}, bound {round_bound(st)}, jump_steps {st['jump_steps']}, present {st['present']}")
    assert st["jump_rounds"] <= round_bound(st)
    x.close()


@pytest.mark.parametrize("which", ["cycle", "cycle2"])
def test_long_cycle(api, which):
    """A 5,000-base unit three times over at k = 15, alone and with its reverse complement as a second record: one circular
    unitig of 5,000 nodes from its lowest 15-mer that occurs, its closing link and the mirror of it as the two edges."""
    E = esa_of(which)
    x = index_of(api, E.records, 32)
    e = x.esa(sa=True, da=True)
    got, st = check(x, e, want_of(which, 15), 15)
    assert got.unitigs["nodes"].tolist() == [5000] and got.unitigs["kmer_count"].tolist() == [14986 * len(E.records)]
    assert got.unitigs["flags"].tolist() == [CR.CIRCULAR] and got.edges.tolist() == [(0, 0), (1, 1)] and st["circular"] == 1
    assert got.strings()[0][:15] == min(s[i:i + 15] for s in F.strings(E.records) for i in range(5000))
    assert st["mated"] == (0 if which == "cycle" else 10000)
    print(f"jump_rounds {st['jump_rounds']}, bound {round_bound(st)}, jump_steps {st['jump_steps']}, present {st['present']}")
    assert st["jump_rounds"] <= round_bound(st)
    x.close()


# ---- hairpins, and edge strings that occur with their reverse complement -----------------------------------------------------

HAND = [(["ACGT"], 3), (["TTACGTCC"], 3), (["ACGTACGTACGT"], 3), (["AACCGTT", "AACGGTT"], 3), (["ACCAGT", "ACTGGT", "CCAGA"], 3),
        (["ACGTACGTACGT", "TTACGTAA"], 3), (["AAAAAAA"], 3), (["AT"], 1), (["ACGGT", "ACCGT"], 1)]


@pytest.mark.parametrize("strs,k", HAND)
def test_hand_collections(api, strs, k):
    recs = codes(strs)
    want = BR.from_esa(ER.Esa(recs), k)
    x = index_of(api, recs, 4)
    e = x.esa(sa=True, da=True)
    got, st = check(x, e, want, k)
    if strs == ["ACGT"]:
        assert st["hairpins"] == 1 and got.strings() == ["ACG"] and got.edges.tolist() == [(0, 1)]
    if len(strs) > 1 and strs[0].startswith("AAC"):
        assert st["edge_keys"] > st["edges"]                                                # the dedup dropped a key
    x.close()


# ---- caps ---------------------------------------------------------------------------------------------------------------

def code_of(api, fn, *args, **kw):
    with pytest.raises(api.DebwtError) as err:
        fn(*args, **kw)
    return err.value.code


@pytest.mark.parametrize("name,k", [("dup_40x20", 7), ("homopolymer_only_one_record", 5), ("n768", 3)])
def test_caps(api, name, k):
    E = ER.of_case(name)
    x = index_of(api, CASES[name], 32)
    e = x.esa(sa=True, da=True)
    full, _ = check(x, e, BR.from_esa(E, k), k)
    e = x.esa(max_lcp=k + 1, sa=True, da=True)
    capped, _ = check(x, e, BR.from_esa(E, k, max_lcp=k + 1), k)
    assert capped.unitigs.tobytes() == full.unitigs.tobytes() and capped.seq.tobytes() == full.seq.tobytes()
    assert capped.edges.tobytes() == full.edges.tobytes()
    e = x.esa(max_lcp=k, sa=True, da=True)
    assert code_of(api, e.cdbg, k, strands="both") == EINVAL
    assert len(e.cdbg(k - 2, strands="both").unitigs) == len(BR.from_esa(E, k - 2).unitigs)
    x.close()


# ---- protocol -----------------------------------------------------------------------------------------------------------

def raw(x, k, un, seq, ed, caps, flags=0, sizes=True):
    from debwt_amd import _lib
    sz = _lib.DebwtFmCdbgSizes(11, 12, 13)
    p = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in (un, seq, ed)]
    rc = x._L.debwt_fm_cdbg_both(x._h, k, flags, p[0], caps[0], p[1], caps[1], p[2], caps[2], ctypes.byref(sz) if sizes else None)
    return rc, (sz.unitigs, sz.seq_bytes, sz.edges)


def test_protocol(api):
    name, k = "n768", 3
    E = ER.of_case(name)
    want = BR.from_esa(E, k)
    U, B, M = want.sizes()
    assert U > 3 and M > 3
    x = index_of(api, CASES[name], 4)
    untouched = (11, 12, 13)
    assert code_of(api, api.EsaResult(x).cdbg, k, strands="both") == ESTATE      # no build
    assert raw(x, k, None, None, None, (0, 0, 0)) == (ESTATE, untouched)
    for kw in ({"sa": True}, {"da": True}, {}):                                  # a build without da, without sa, without both
        e = x.esa(**kw)
        assert code_of(api, e.cdbg, k, strands="both") == ESTATE and raw(x, k, None, None, None, (0, 0, 0)) == (ESTATE, untouched)
    e = x.esa(sa=True, da=True)
    lcp0, sa0, da0, b0 = e.lcp(), e.sa(), e.da(), x.info()["device_bytes"]
    un, seq, ed = np.zeros(U + 1, dtype=CR.UNITIG_DTYPE), np.zeros(B + 1, dtype=np.uint8), np.zeros(M + 1, dtype=CR.EDGE_DTYPE)
    clean = lambda: not un.view(np.uint8).any() and not seq.any() and not ed.view(np.uint8).any()   # noqa: E731
    assert raw(x, 0, un, seq, ed, (U, B, M)) == (EINVAL, untouched)              # k = 0
    for even in (2, 4, 1000):
        assert raw(x, even, un, seq, ed, (U, B, M)) == (EINVAL, untouched)       # an even k
    assert raw(x, k, un, seq, ed, (U, B, M), flags=1) == (EINVAL, untouched)
    assert raw(x, k, un, seq, ed, (U, B, M), sizes=False)[0] == EINVAL
    for caps in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):                               # a NULL array with capacity > 0
        assert raw(x, k, None, None, None, caps) == (EINVAL, untouched)
    assert clean()
    assert raw(x, k, None, None, None, (0, 0, 0)) == (ERANGE, (U, B, M))         # the sizing call
    for caps in ((U - 1, B, M), (U, B - 1, M), (U, B, M - 1)):                   # each capacity one short
        assert raw(x, k, un, seq, ed, caps) == (ERANGE, (U, B, M)), caps
        assert clean()
    assert raw(x, k, un, seq, ed, (U, B, M)) == (0, (U, B, M))
    assert np.array_equal(un[:U], want.unitigs) and np.array_equal(seq[:B], want.seq) and np.array_equal(ed[:M], want.edges)
    assert not un[U:].view(np.uint8).any() and not seq[B:].any() and not ed[M:].view(np.uint8).any()
    assert raw(x, k, un, seq, ed, (U + 1, B + 1, M + 1)) == (0, (U, B, M))
    assert raw(x, 2001, None, None, None, (0, 0, 0)) == (0, (0, 0, 0))            # every record is shorter: all sizes 0
    assert np.array_equal(e.lcp(), lcp0) and np.array_equal(e.sa(), sa0) and np.array_equal(e.da(), da0)
    assert x.info()["device_bytes"] == b0
    with pytest.raises(ValueError):
        e.cdbg(k, strands="reverse")
    e.release()
    assert code_of(api, e.cdbg, k, strands="both") == ESTATE
    x.close()


def test_even_k_says_why(api):
    x = index_of(api, CASES["n768"], 4)
    e = x.esa(sa=True, da=True)
    with pytest.raises(api.DebwtError) as err:
        e.cdbg(4, strands="both")
    assert err.value.code == EINVAL and "odd" in str(err.value)
    x.close()


# ---- the forward call is what it was ----------------------------------------------------------------------------------------

def test_forward_call_is_untouched(api):
    E = esa_of("pan")
    x = index_of(api, E.records, 32)
    e = x.esa(sa=True, da=True)
    lcp0, sa0, da0 = e.lcp(), e.sa(), e.da()
    before = e.cdbg(21)
    st0 = {n: v for n, v in x.cdbg_stats().items() if n in CR.COUNTING}
    both = e.cdbg(21, strands="both")
    after = e.cdbg(21)
    assert after.strands == "forward" and len(both.unitigs) == 487
    assert before.unitigs.tobytes() == after.unitigs.tobytes() and before.seq.tobytes() == after.seq.tobytes()
    assert before.edges.tobytes() == after.edges.tobytes()
    assert {n: v for n, v in x.cdbg_stats().items() if n in CR.COUNTING} == st0
    CR.same_graph(CR.Cdbg(21, after.unitigs, after.seq, after.edges, st0), CR.from_esa(E, 21))
    assert np.array_equal(e.lcp(), lcp0) and np.array_equal(e.sa(), sa0) and np.array_equal(e.da(), da0)
    x.close()
