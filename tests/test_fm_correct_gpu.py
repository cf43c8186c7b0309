"""k-mer read correction on the device (debwt_fm_correct, FMIndex.correct) against the reference of kmer_ref.py: the output
reads and every info field, bit for bit, on the seeded read set with the reads made for one case each
(test_fm_kmer_ref.py asserts that the reference alone meets every case); rounds, strands, batch limits and table sizes,
short and empty reads, errors and statistics."""
import ctypes

import numpy as np
import pytest

import kmer_ref as KR
from overlap_ref import codes
from test_fm_search_gpu import index_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


@pytest.fixture(scope="module")
def fm(api):
    """the index of the seeded read set: built once, queried by every test below and never changed"""
    x = index_of(api, codes(KR.read_set()["records"]), s=4)
    yield x
    x.close()


@pytest.fixture(autouse=True)
def default_limits(monkeypatch):
    monkeypatch.delenv("DEBWT_FM_KMER_TABLE_Q", raising=False)
    monkeypatch.delenv("DEBWT_FM_KMER_ITEMS", raising=False)


def check(got, want, pats):
    reads, info = got
    assert len(reads) == len(info) == len(want) == len(pats)
    for i, w in enumerate(want):
        assert reads[i].decode() == w[0], (i, pats[i])
        assert tuple(int(x) for x in info[i]) == w[1:5], (i, pats[i])


@pytest.mark.parametrize("rounds", [1, 4])
@pytest.mark.parametrize("strands", ["forward", "both"])
@pytest.mark.parametrize("k,min_count", [(15, 3), (21, 2)])
def test_read_set(api, fm, k, min_count, strands, rounds):
    pats = KR.correction_queries(k)
    want = KR.corrected(k, min_count, strands == "both", rounds)
    if rounds == 4:                                             # one round is not enough for every read
        one = KR.corrected(k, min_count, strands == "both", 1)
        assert any(a[:5] != b[:5] for a, b in zip(one, want))
    got = fm.correct(pats, k, min_count=min_count, rounds=rounds, strands=strands)
    check(got, want, pats)
    st = fm.correct_stats()
    info = got[1]
    assert st["fixes"] == int(info["fixes"].sum()) > 0 and st["patterns"] == len(pats)
    per = {f: int((info["flags"] == f).sum()) for f in (api.CORRECT_SHORT, api.CORRECT_CLEAN, api.CORRECT_FIXED, api.CORRECT_WEAK)}
    assert sum(per.values()) == len(pats) and min(per.values()) > 0
    assert (st["reads_short"], st["reads_clean"], st["reads_fixed"], st["reads_weak"]) == tuple(per.values())
    assert 1 <= st["rounds"] <= rounds and st["trials"] >= st["fixes"]
    assert sum(st["active"]) >= int((info["fixes"] > 0).sum()) and all(a == 0 for a in st["active"][st["rounds"]:])
    assert 0 < st["steps"] <= st["wave_steps"] and st["line_reads"] >= st["steps"] and st["ms_kernel"] > 0
    assert st["batches"] == 1 and st["scratch_bytes"] > 0 and st["kmers"] >= int(info["weak_before"].sum() > 0)


def test_limits_do_not_change_the_bytes(api, fm, monkeypatch):
    k = 15
    pats = KR.correction_queries(k)
    want = KR.corrected(k, 3, True, 4)
    for items, q in (("7", None), ("500", "0"), (None, "6"), ("90", "6")):
        for name, v in (("DEBWT_FM_KMER_ITEMS", items), ("DEBWT_FM_KMER_TABLE_Q", q)):
            monkeypatch.setenv(name, v) if v else monkeypatch.delenv(name, raising=False)
        got = fm.correct(pats, k)
        check(got, want, pats)
        st = fm.correct_stats()
        assert (st["batches"] > 1) == bool(items) and st["table_q"] == (int(q) if q else 12)
        assert st["fixes"] == int(got[1]["fixes"].sum())


def test_short_empty_and_case(api, fm):
    k = 15
    g = KR.read_set()["genome"]
    low = g[820:880].lower()
    pats = ["", "ACGT", g[100:100 + k - 1], low, g[900:960], "n" * 40]
    reads, info = fm.correct(pats, k)
    assert [r.decode() for r in reads] == pats
    assert info["flags"].tolist() == [1, 1, 1, 2, 2, 8] and info["fixes"].sum() == 0
    assert info["weak_before"].tolist() == [0, 0, 0, 0, 0, 40 - k + 1] == info["weak_after"].tolist()
    reads, info = fm.correct(["", "ACG"], k)                    # a batch of short reads alone
    assert reads == [b"", b"ACG"] and info["flags"].tolist() == [1, 1]
    assert fm.correct([], k)[0] == []
    # a fix is written in upper case, every other byte stays as given
    j = 31
    bad = low[:j] + ("a" if low[j] != "a" else "c") + low[j + 1:]
    reads, info = fm.correct([bad], k)
    assert reads[0].decode() == low[:j] + low[j].upper() + low[j + 1:] and tuple(info[0]) == (4, 1, k, 0)


def test_errors(api, fm):
    from debwt_amd import _lib
    for kw in ({"k": 0}, {"k": 15, "min_count": 0}, {"k": 15, "rounds": 0}, {"k": 15, "rounds": 17}):
        with pytest.raises(api.DebwtError) as e:
            fm.correct(["ACGTACGTACGTACGTACGT"], **kw)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        fm.correct(["ACGT"], 15, strands="reverse")
    L = _lib.lib()
    buf = b"ACGTACGTACGTACGTACGT"
    offs = np.array([0, len(buf)], dtype=np.uint64)
    out = ctypes.create_string_buffer(len(buf))
    info = (_lib.DebwtFmCorrectInfo * 1)()
    for flags in (2, 4 | 1):
        o = _lib.DebwtFmCorrectOpts(k=15, min_count=3, max_rounds=4, flags=flags)
        assert L.debwt_fm_correct(fm._h, buf, api._p64(offs), 1, ctypes.byref(o), out, info) == -1
    o = _lib.DebwtFmCorrectOpts(k=15, min_count=3, max_rounds=4, flags=1)
    bad = np.array([5, 0], dtype=np.uint64)
    assert L.debwt_fm_correct(fm._h, buf, api._p64(bad), 1, ctypes.byref(o), out, info) == -1
    assert L.debwt_fm_correct(fm._h, buf, api._p64(offs), 1, None, out, info) == -1
    assert L.debwt_fm_correct(fm._h, buf, api._p64(offs), 1, ctypes.byref(o), out, info) == 0
