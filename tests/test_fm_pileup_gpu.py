"""Pileup, calls, insertion events and consensus on the GPU (debwt_fm_pileup, debwt_fm_pile_call,
debwt_fm_pile_insertions) against tests/pileup_ref.py, which writes definitions 7 and 8 of include/debwt_hip.h out
literally.  Everything is integers and strings, so every comparison is exact.  Every table is made by both counting
forms (DEBWT_PILE_FORM) and must be the same."""
import ctypes

import numpy as np
import pytest

import pileup_ref as R
from test_fm_pileup_ref import rand_dna, random_input

pytestmark = pytest.mark.gpu
FORMS = ["lane", "group16", "group64", ""]
EINVAL, ESTATE, ERANGE = -1, -4, -5


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def codes(s):
    return np.array([R.SLOT[c] for c in s], dtype=np.uint8)


def index_of(api, strs, s=8, text=True):
    d = api.DeBWT(k=32)
    d.load_records([codes(x) for x in strs])
    d.build()
    fm = d.fm_index(sa_sample=s)
    if text:
        fm.attach_text(d)
    d.close()
    return fm


def pack(api, alns, cigars):
    rows = np.array([tuple(a) for a in alns], dtype=api._PILE_ALN_DTYPE) if alns else np.zeros(0, dtype=api._PILE_ALN_DTYPE)
    coff = np.zeros(len(alns) + 1, dtype=np.uint64)
    if alns:
        np.cumsum([len(c) for c in cigars], out=coff[1:])
    cg = np.array([x for c in cigars for x in c], dtype=np.uint32)
    return rows, coff, cg


def unpack(packed):
    rows, coff, cg = packed
    alns = [tuple(int(x) for x in r) for r in rows.tolist()]
    cigars = [[int(x) for x in cg[int(coff[g]):int(coff[g + 1])]] for g in range(len(alns))]
    return alns, cigars


def var_tuples(v):
    return [tuple(int(x) for x in r) for r in v.tolist()]


def compare(api, monkeypatch, fm, strs, pats, alns, cigars, window=None, min_depth=4, min_permille=600, forms=FORMS):
    """table (by every form), calls, variants, events, voted strings and consensus against the reference"""
    text, starts = R.text_of(strs)
    window = window or (0, len(text))
    table, calls, variants, voted, cons = R.run(pats, alns, cigars, strs, window, min_depth, min_permille)
    want = np.array(table, dtype=np.uint32).reshape(-1, 8)
    for form in forms:
        monkeypatch.setenv("DEBWT_PILE_FORM", form)
        res = fm.pileup(pats, pack(api, alns, cigars), window=window)
        assert np.array_equal(res.counts, want), form
        st = fm.pile_stats()
        assert st["group"] == {"lane": 1, "group16": 16, "group64": 64}.get(form, st["group"])
    monkeypatch.delenv("DEBWT_PILE_FORM")
    assert np.array_equal(res.depth, want[:, :5].sum(axis=1))
    cr = res.call(min_depth, min_permille)
    assert cr.calls.tolist() == calls
    assert cr.ref.tolist() == [R.SLOT.get(c, 4) for c in text[window[0]:window[1]]]
    assert var_tuples(cr.variants) == variants
    flagged = [v[0] for v in variants if v[5] & R.INS_BIT]
    ev = fm.pile_insertions(pats, pack(api, alns, cigars), flagged)
    assert var_tuples(ev) == R.insertions(pats, alns, cigars, flagged)
    assert {t: (s, sup, d) for t, s, sup, d in cr.insertions()} == voted
    got = dict(cr.consensus())
    for r, s in enumerate(cons):
        assert got.get(r, "") == s
    return res, cr


@pytest.fixture(scope="module")
def crafted(api):
    """records of 1,000, 21,000 and 400 b and their index: made once, never changed"""
    rng = np.random.default_rng(23)
    strs = [rand_dna(rng, 1000), rand_dna(rng, 21000), rand_dna(rng, 400)]
    return strs, index_of(api, strs)


def mutate(rng, s, p_sub=0.03, p_indel=0.01):
    out = []
    for c in s:
        r = rng.random()
        if r < p_sub:
            out.append("ACGT"[(R.SLOT[c] + int(rng.integers(1, 4))) % 4])
        elif r < p_sub + p_indel / 2:
            continue
        elif r < p_sub + p_indel:
            out.append(c)
            out.append(rand_dna(rng, int(rng.integers(1, 3))))
        else:
            out.append(c)
    return "".join(out)


@pytest.mark.parametrize("seed", [5, 6])
def test_random_collections_extend_and_map(api, monkeypatch, seed):
    rng = np.random.default_rng(seed)
    strs = [rand_dna(rng, int(rng.integers(300, 2001))) for _ in range(3)]
    text, starts = R.text_of(strs)
    fm = index_of(api, strs)
    reads, jobs = [], []
    for g in range(400):
        r = int(rng.integers(0, 3))
        m = int(rng.integers(8, 151))
        a = int(rng.integers(0, len(strs[r]) - m + 1))
        read = mutate(rng, strs[r][a:a + m]) or "A"
        strand = int(rng.integers(0, 2))
        if strand:
            read = R.query(read, 1)
        if g % 9 == 0:
            read = read.lower()
        if g % 11 == 0:
            read = read[:len(read) // 2] + "N" + read[len(read) // 2 + 1:]
        reads.append(read)
        jobs.append((g, strand, starts[r] + a, r))             # the planted diagonal: query position 0 at text a
    ext = fm.extend(reads, jobs, band=16)
    alns, cigars = unpack(ext.alignments(jobs))
    assert len(alns) > 300 and any(x & 15 == 1 for c in cigars for x in c) and any(x & 15 == 2 for c in cigars for x in c)
    compare(api, monkeypatch, fm, strs, reads, alns, cigars, min_depth=2)
    mp = fm.map(reads)
    alns, cigars = unpack(mp.alignments())
    assert len(alns) > 200 and any(a[3] for a in alns) and any(a[2] for a in alns)
    res, _ = compare(api, monkeypatch, fm, strs, reads, alns, cigars, min_depth=2, forms=["lane", ""])
    # the same through MapResult.pileup, with a quality cut and a window
    win = (starts[1], starts[1] + 200)
    keep = mp.mapped & (mp.mapq >= 20)
    a20, c20 = unpack(mp.alignments(20))
    assert len(a20) == int(keep.sum())
    got = mp.pileup(fm, reads, min_mapq=20, window=win).counts
    assert np.array_equal(got, np.array(R.dense(R.pileup(reads, a20, c20, len(text), win), win), dtype=np.uint32))
    fm.close()


@pytest.mark.parametrize("cols", [1, 15, 16, 17, 63, 64, 65, 129, 300])
def test_one_match_op_at_the_group_edges(api, monkeypatch, crafted, cols):
    strs, fm = crafted
    rng = np.random.default_rng(cols)
    pats = [rand_dna(rng, cols + 7, "ACGTNacgt"), rand_dna(rng, cols)]
    # strand 1 with qbeg > 0, and a read that is all of its CIGAR; both forms see the same codes
    compare(api, monkeypatch, fm, strs, pats, [(0, 100, 5, 1), (1, 333, 0, 0), (0, 1000 - cols, 2, 0)],
            [[cols << 4]] * 3, min_depth=1)


def test_many_short_ops_and_a_long_read(api, monkeypatch, crafted):
    strs, fm = crafted
    rng = np.random.default_rng(7)
    zig = []
    for k in range(75):
        zig += [1 << 4, 1 << 4 | 1, 1 << 4, 1 << 4 | 2]
    zig.append(1 << 4)                                         # 301 ops: 1M1I1M1D ... 1M, 226 query bases, 226 text positions
    assert len(zig) == 301
    long_ops, left = [], 20000
    for k in range(40):
        ln = 300 + 7 * k
        long_ops += [ln << 4, ((k % 5 + 1) << 4) | (1 if k % 2 else 2)]
        left -= ln + (k % 5 + 1 if k % 2 else 0)
    long_ops.append(left << 4)
    pats = [rand_dna(rng, 226 + 3, "ACGTN"), rand_dna(rng, 20000)]
    alns = [(0, 40, 3, 1), (0, 500, 0, 0), (1, 1001 + 17, 0, 1), (1, 1001 + 500, 0, 0)]
    compare(api, monkeypatch, fm, strs, pats, alns, [zig, zig, long_ops, long_ops], min_depth=1)
    st = fm.pile_stats()
    assert st["alignments"] == 4 and st["ops"] == 2 * 301 + 2 * 81 and st["i_ops"] == 2 * 75 + 2 * 20


def test_windows(api, monkeypatch, crafted):
    strs, fm = crafted
    rng = np.random.default_rng(8)
    pats = [rand_dna(rng, 120, "ACGTNacgt") for _ in range(4)]
    #  M 30, D 5, M 30, I 3, M 57: text 122 from tbeg; the deletion covers tbeg + 30 .. + 34, the insertion sits at tbeg + 64
    ops = [30 << 4, 5 << 4 | 2, 30 << 4, 3 << 4 | 1, 57 << 4]
    alns = [(0, 200, 0, 0), (1, 210, 0, 1), (2, 190, 0, 0), (3, 205, 0, 1)]
    cig = [ops] * 4
    for win in [(230, 300),                                    # begins before wbeg, ends after wend
                (232, 260),                                    # the deletion of alignment 0 crosses wbeg
                (200, 265), (265, 300),                        # alignment 0's insertion at wend - 1: counted; at wbeg - 1: not
                (264, 265), (233, 234), (0, 1),                # windows of one position
                (100, 400)]:
        res, _ = compare(api, monkeypatch, fm, strs, pats, alns, cig, window=win, min_depth=1, forms=["lane", ""])
        if win == (200, 265):
            assert res.counts[64, 5] == 1
        if win == (265, 300):
            assert res.counts[:, 5].sum() == sum(1 for a in alns[1:] if 265 <= a[1] + 64 < 300)


def test_nothing_to_count(api, crafted):
    strs, fm = crafted
    res = fm.pileup(["ACGT"], pack(api, [], []), window=(10, 50))
    assert res.counts.shape == (40, 8) and not res.counts.any()
    assert fm.pile_stats()["alignments"] == 0
    # an alignment with an empty CIGAR contributes nothing, whatever stands beside it
    res = fm.pileup(["ACGT"], pack(api, [(0, 0, 0, 0), (0, 12, 0, 0), (0, 0, 0, 0)], [[], [4 << 4], []]), window=(10, 50))
    assert res.counts.sum() == 4 and res.counts[2:6, :4].sum() == 4
    calls, ref, var = fm.pile_call()
    assert set(calls.tolist()) == {R.NO_CALL} and len(var) == 0


def test_contention(api, monkeypatch, crafted):
    strs, fm = crafted
    read = strs[0][300:400]
    alns, cig = [(0, 300, 0, 0)] * 5000, [[100 << 4]] * 5000
    for form in FORMS:
        monkeypatch.setenv("DEBWT_PILE_FORM", form)
        c = fm.pileup([read], pack(api, alns, cig), window=(250, 450)).counts
        assert c.sum() == 500000 and (c[50:150].sum(axis=1) == 5000).all() and (c[50:150].max(axis=1) == 5000).all()
        assert not c[:50].any() and not c[150:].any()


def test_batches_add_up(api, crafted):
    strs, fm = crafted
    _, text, pats, alns, cigars = random_input(4, naln=70)
    n = len(R.text_of(strs)[0])
    want = np.array(R.dense(R.pileup(pats, alns, cigars, n, (0, 900)), (0, 900)), dtype=np.uint32)
    for nb in (1, 2, 7):
        step = (len(alns) + nb - 1) // nb
        for k, a in enumerate(range(0, len(alns), step)):
            res = fm.pileup(pats, pack(api, alns[a:a + step], cigars[a:a + step]), window=(0, 900), add=k > 0)
        assert np.array_equal(res.counts, want), nb
    # without the flag a call clears; with the flag and another window it is refused and the table stays
    one = fm.pileup(pats, pack(api, alns[:1], cigars[:1]), window=(0, 900)).counts
    assert np.array_equal(one, np.array(R.dense(R.pileup(pats, alns[:1], cigars[:1], n, (0, 900)), (0, 900)), dtype=np.uint32))
    with pytest.raises(api.DebwtError) as e:
        fm.pileup(pats, pack(api, alns, cigars), window=(0, 901), add=True)
    assert e.value.code == EINVAL
    assert np.array_equal(fm.pile_fetch()[1], one)
    fm.pile_release()
    with pytest.raises(api.DebwtError) as e:
        fm.pile_fetch()
    assert e.value.code == ESTATE
    res = fm.pileup(pats, pack(api, alns, cigars), window=(0, 900), add=True)      # no table: the flag changes nothing
    assert np.array_equal(res.counts, want)


def hand_alignments(text, spec):
    """alignments that put at least spec[t] = (a, c, g, t, del, ins, other) on position t: reads of one base for the
    base slots, xMyDzM for a deletion, 1M1I1M for an insertion (these also touch the neighbours of t)"""
    pats, alns, cig = [], [], []
    for t, c in sorted(spec.items()):
        c = list(c) + [0] * (7 - len(c))
        for slot, ch in ((0, "A"), (1, "C"), (2, "G"), (3, "T"), (6, "N")):
            for _ in range(c[slot]):
                pats.append(ch)
                alns.append((len(pats) - 1, t, 0, 0))
                cig.append([1 << 4])
        for _ in range(c[4]):
            pats.append("NN")
            alns.append((len(pats) - 1, t - 1, 0, 0))
            cig.append([1 << 4, 1 << 4 | 2, 1 << 4])
        for _ in range(c[5]):
            pats.append("NAN")
            alns.append((len(pats) - 1, t, 0, 0))
            cig.append([1 << 4, 1 << 4 | 1, 1 << 4])
    return pats, alns, cig


def test_call_clauses(api, monkeypatch, crafted):
    strs, fm = crafted
    text, starts = R.text_of(strs)
    def at(ch, frm):
        return text.index(ch, frm)
    a1, c1, g1 = at("A", 100), at("C", 120), at("G", 140)
    sep = starts[1] - 1
    spec = {
        a1: (0, 4),                  # depth = min_depth, all C over an A: a substitution
        90: (0, 3),                  # depth = min_depth - 1: no call
        c1: (2, 3),                  # 3 of 5: exactly on the 600 line, called C = ref, no variant
        95: (402, 598),              # 598 of 1000: one below the line at this depth
        g1: (2, 2),                  # tie A / C at a G: below the line at 600, the lowest tied slot at 500
        at("C", 160): (3, 3),        # tie that holds the reference base
        at("T", 180): (0, 0, 0, 1, 4),   # a called deletion
        at("T", 200): (0, 0, 0, 3, 3),   # tie of the reference base and a deletion
        sep: (6,),                   # a separator covered by alignments: never called
        at("A", 220): (5, 0, 0, 0, 0, 3),    # 3 insertions over a depth of 5: exactly on the line
        at("A", 230): (5, 0, 0, 0, 0, 2),    # 2 over 5: below it
        at("A", 240): (4, 0, 0, 0, 0, 6),    # the insertion bit, more insertions than depth
        at("A", 260): (0, 1, 0, 0, 0, 9, 30),   # insertions and other characters at a position that is not called
    }
    pats, alns, cig = hand_alignments(text, spec)
    for md, mp in [(4, 600), (4, 500), (1, 1000), (5, 0)]:
        res, cr = compare(api, monkeypatch, fm, strs, pats, alns, cig, window=(50, 1100), min_depth=md, min_permille=mp,
                          forms=["lane", ""])
    res, cr = compare(api, monkeypatch, fm, strs, pats, alns, cig, window=(50, 1100), forms=[""])
    call = {t: int(cr.calls[t - 50]) for t in spec}
    assert call[a1] == 1 and call[90] == R.NO_CALL and call[c1] == 1 and call[95] == R.NO_CALL
    assert call[g1] == R.NO_CALL and call[sep] == R.NO_CALL and int(cr.ref[sep - 50]) == 4
    assert call[at("T", 180)] == R.DEL and call[at("T", 200)] == R.NO_CALL
    assert call[at("A", 220)] == R.INS_BIT and call[at("A", 230)] == 0
    assert call[at("A", 240)] == R.INS_BIT and call[at("A", 260)] == R.NO_CALL
    assert a1 in cr.variants["t"].tolist() and c1 not in cr.variants["t"].tolist()
    at500 = fm.pile_call(4, 500)[0]
    assert at500[g1 - 50] == 0 and at500[at("T", 200) - 50] == 3 and at500[at("C", 160) - 50] == 1


def test_variant_positions_and_capacity(api, crafted):
    strs, fm = crafted
    text, _ = R.text_of(strs)
    L, h = fm._L, fm._h
    from debwt_amd import _lib
    def wrong(t):
        return "ACGT"[(R.SLOT[text[t]] + 1) % 4]
    wbeg = 77
    for offs in ([0, 63, 64, 65], [599], [0, 255, 256, 511, 512, 599], []):
        pats, alns, cig = [], [], []
        for o in offs:
            for _ in range(4):
                pats.append(wrong(wbeg + o))
                alns.append((len(pats) - 1, wbeg + o, 0, 0))
                cig.append([1 << 4])
        fm.pileup(pats or ["A"], pack(api, alns, cig), window=(wbeg, wbeg + 600))
        calls = np.zeros(600, dtype=np.uint8)
        nv = ctypes.c_uint64(99)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        rc = L.debwt_fm_pile_call(h, None, calls.ctypes.data_as(u8p), None, None, 0, ctypes.byref(nv))
        assert rc == (ERANGE if offs else 0) and nv.value == len(offs)
        assert [i for i, c in enumerate(calls.tolist()) if c != R.NO_CALL] == offs      # the calls were written first
        var = np.zeros(max(len(offs), 1), dtype=api._VARIANT_DTYPE)
        rc = L.debwt_fm_pile_call(h, None, calls.ctypes.data_as(u8p), None,
                                  var.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmVariant)), len(offs), ctypes.byref(nv))
        assert rc == 0 and nv.value == len(offs)
        assert var["t"][:len(offs)].tolist() == [wbeg + o for o in offs]
        assert all(int(v["depth"]) == 4 and int(v["count"]) == 4 and int(v["call"]) != int(v["ref"]) for v in var[:len(offs)])


def test_insertion_events(api, crafted):
    strs, fm = crafted
    rng = np.random.default_rng(9)
    pats, alns, cig = [], [], []
    def add(t, n, ops=None):
        for _ in range(n):
            pats.append(rand_dna(rng, 40))
            alns.append((len(pats) - 1, t - 9, 0, int(rng.integers(0, 2))))
            cig.append(ops or [10 << 4, int(rng.integers(1, 4)) << 4 | 1, 10 << 4])
    add(300, 1)
    add(400, 64)
    add(500, 65)
    add(600, 3, [10 << 4, 2 << 4 | 1, 5 << 4, 1 << 4 | 1, 5 << 4, 3 << 4 | 1, 4 << 4])   # I ops at 600, 605 and 610
    packed = pack(api, alns, cig)
    for listed in ([200, 300, 400, 500], [300], [600, 610], [605], [250], [], [299, 301, 399, 401, 604, 606]):
        ev = fm.pile_insertions(pats, packed, listed)
        want = R.insertions(pats, alns, cig, listed)
        assert var_tuples(ev) == want, listed
    assert len(fm.pile_insertions(pats, packed, [200, 300, 400, 500])) == 130
    assert len(fm.pile_insertions(pats, packed, [600, 610])) == 6
    # the capacity protocol
    from debwt_amd import _lib
    rows, coff, cg = api._pile_alns(packed)
    _, offs = api._patterns(pats)
    pos = np.array([400], dtype=np.uint64)
    ne = ctypes.c_uint64(0)
    evb = np.zeros(64, dtype=api._INS_EVENT_DTYPE)
    args = (fm._h, len(pats), api._p64(offs), rows.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmPileAln)), len(alns), api._p64(coff),
            cg.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), api._p64(pos), 1)
    evp = evb.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmInsEvent))
    assert fm._L.debwt_fm_pile_insertions(*args, evp, 63, ctypes.byref(ne)) == ERANGE and ne.value == 64
    assert fm._L.debwt_fm_pile_insertions(*args, evp, 64, ctypes.byref(ne)) == 0 and ne.value == 64
    assert var_tuples(evb) == R.insertions(pats, alns, cig, [400])


def test_index_from_files_restores_the_text(api, monkeypatch):
    rng = np.random.default_rng(10)
    strs = [rand_dna(rng, 500), rand_dna(rng, 333)]
    d = api.DeBWT(k=32)
    d.load_records([codes(x) for x in strs])
    d.build()
    words, hrows, drow = d.fetch()
    own = d.fm_index(sa_sample=4)
    opened = api.FMIndex.open(words, own.n, hrows, drow, own.samples(), sa_sample=4)
    d.close()
    _, text, pats, alns, cigars = random_input(11, naln=50)
    alns = [(p, t % 600, q, s) for p, t, q, s in alns]
    before = opened.info()["device_bytes"]
    compare(api, monkeypatch, opened, strs, pats, alns, cigars, min_depth=1, forms=[""])
    assert opened.info()["device_bytes"] > before + 32 * own.n             # the table and the restored text are counted
    own.close()
    opened.close()


def test_refusals_leave_the_table(api, crafted):
    strs, fm = crafted
    n = fm.n
    pats = ["ACGTACGTAC", "ACGT"]
    good = ([(0, 5, 0, 0), (1, 8, 0, 1)], [[10 << 4], [4 << 4]])
    keep = fm.pileup(pats, pack(api, *good), window=(0, 64)).counts.copy()
    assert keep.sum() == 14
    M = lambda k: k << 4
    bad = [
        ([(0, 5, 0, 0)], [[M(3) | 3]], (0, 64)),               # an op code above 2
        ([(0, 5, 0, 0)], [[M(3), 0 << 4 | 1, M(3)]], (0, 64)),  # an op of length 0
        ([(0, 5, 0, 0)], [[M(1) | 1, M(5)]], (0, 64)),          # begins with I
        ([(0, 5, 0, 0)], [[M(5), M(1) | 2]], (0, 64)),          # ends with D
        ([(2, 5, 0, 0)], [[M(4)]], (0, 64)),                    # pattern >= npat
        ([(0, 5, 0, 2)], [[M(4)]], (0, 64)),                    # strand > 1
        ([(0, 5, 1, 0)], [[M(10)]], (0, 64)),                   # query bases past the read
        ([(0, 5, 0, 0)], [[M(5), M(2) | 1, M(4)]], (0, 64)),    # the same through an insertion
        ([(0, n - 9, 0, 0)], [[M(10)]], (0, 64)),               # text past n
        ([(0, n - 11, 0, 0)], [[M(5), M(2) | 2, M(5)]], (0, 64)),   # the same through a deletion
        (good[0], good[1], (64, 64)), (good[0], good[1], (70, 64)), (good[0], good[1], (0, n + 1)),
        (good[0] + [(0, 5, 0, 0)], good[1] + [[M(11)]], (0, 64)),   # one bad alignment behind good ones
    ]
    for alns, cig, win in bad:
        for add in (False, True):
            with pytest.raises(api.DebwtError) as e:
                fm.pileup(pats, pack(api, alns, cig), window=win, add=add)
            assert e.value.code == EINVAL, (alns, cig, win)
            assert np.array_equal(fm.pile_fetch()[1], keep)
        if win == (0, 64):
            with pytest.raises(R.Invalid):
                R.pileup(pats, alns, cig, n, win)
    # what is just inside: the last text position, the whole read
    fm.pileup(pats, pack(api, [(0, n - 10, 0, 0), (1, 0, 0, 1)], [[M(10)], [M(4)]]), window=(n - 1, n))
    # fetch: the capacity protocol
    win = np.zeros(2, dtype=np.uint64)
    buf = np.zeros((1, 8), dtype=np.uint32)
    assert fm._L.debwt_fm_pile_fetch(fm._h, api._p64(win), buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 0) == ERANGE
    assert win.tolist() == [n - 1, n] and not buf.any()
    assert fm._L.debwt_fm_pile_fetch(fm._h, api._p64(win), buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 1) == 0


def test_statistics(api, monkeypatch, crafted):
    strs, fm = crafted
    _, text, pats, alns, cigars = random_input(12, naln=80)
    ops = [x for c in cigars for x in c]
    for form, group in (("lane", 1), ("group16", 16), ("", 16)):
        monkeypatch.setenv("DEBWT_PILE_FORM", form)
        res = fm.pileup(pats, pack(api, alns, cigars), window=(100, 700))
        st = fm.pile_stats()
        c = res.counts.sum(axis=0, dtype=np.uint64)
        assert st["alignments"] == 80 and st["ops"] == len(ops) and st["group"] == group
        assert st["m_columns"] == sum(x >> 4 for x in ops if x & 15 == 0)
        assert st["d_bases"] == sum(x >> 4 for x in ops if x & 15 == 2) and st["i_ops"] == sum(1 for x in ops if x & 15 == 1)
        assert (st["ev_base"], st["ev_other"], st["ev_del"], st["ev_ins"]) == (int(c[:4].sum()), int(c[6]), int(c[4]), int(c[5]))
        assert st["launches"] == 3 and st["ms_kernel"] > 0 and st["ms_wall"] > 0 and st["table_bytes"] == 600 * 32
    fm.pile_call()
    st = fm.pile_stats()
    assert st["call_positions"] == 600 and st["ms_call"] > 0 and st["alignments"] == 80


def test_mapper_is_untouched_by_a_pileup(api, crafted):
    strs, fm = crafted
    reads = [strs[0][a:a + 90] for a in range(0, 900, 45)] + [strs[1][a:a + 120] for a in range(0, 3000, 150)]
    def snapshot():
        m = fm.map(reads, strands="forward")
        st = fm.extend_stats()
        return m.hits.tobytes(), m.offsets.tobytes(), m.cigars.tobytes(), {k: v for k, v in st.items() if not k.startswith("ms_")}
    before = snapshot()
    m = fm.map(reads, strands="forward")
    m.pileup(fm, reads).call()
    assert snapshot() == before


# ---- end to end: planted edits come back as the variants, the consensus is the edited copy --------------------------------

E2E_SEED = 1


def planted_case(seed):
    """3 records of 3 to 5 kb; a copy with 6 substitutions, deletions of 1 and 3 b and insertions of 1 and 4 b, at least
    100 b apart and 150 b from record ends, every indel placed uniquely; reads of 100 b every 5 b of the copy, alternating
    strands.  Returns (records, copies, reads, planted) with planted = {global position: (kind, string)} in the
    coordinates of the original: ('sub', base), ('del', '') per deleted position, ('ins', string) at the anchor."""
    rng = np.random.default_rng(seed)
    strs = [rand_dna(rng, int(rng.integers(3000, 5001))) for _ in range(3)]
    _, starts = R.text_of(strs)
    kinds = ["sub"] * 6 + ["del1", "del3", "ins1", "ins4"]
    planted, edits = {}, [[] for _ in strs]
    used = [[] for _ in strs]
    for k, kind in enumerate(kinds):
        r = k % 3
        s = strs[r]
        while True:
            p = int(rng.integers(150, len(s) - 160))
            if any(abs(p - u) < 110 for u in used[r]):
                continue
            if kind == "sub":
                new = "ACGT"[(R.SLOT[s[p]] + int(rng.integers(1, 4))) % 4]
                edits[r].append((p, 1, new))
                planted[starts[r] + p] = ("sub", new)
            elif kind.startswith("del"):
                L = int(kind[3])
                if s[p] == s[p + L] or s[p + L - 1] == s[p - 1]:
                    continue
                edits[r].append((p, L, ""))
                for x in range(L):
                    planted[starts[r] + p + x] = ("del", "")
            else:
                L = int(kind[3])
                ins = rand_dna(rng, L)
                if ins[0] == s[p + 1] or ins[-1] == s[p]:      # inserted behind position p
                    continue
                edits[r].append((p + 1, 0, ins))
                planted[starts[r] + p] = ("ins", ins)
            used[r].append(p)
            break
    copies = []
    for r, s in enumerate(strs):
        out, at = [], 0
        for p, L, new in sorted(edits[r]):
            out.append(s[at:p])
            out.append(new)
            at = p + L
        out.append(s[at:])
        copies.append("".join(out))
    reads = []
    for c in copies:
        for k, a in enumerate(range(0, len(c) - 99, 5)):
            reads.append(c[a:a + 100] if k % 2 == 0 else R.query(c[a:a + 100], 1))
    return strs, copies, reads, planted


def found_set(variants, voted):
    """variants as {position: (kind, string)}: a position with the insertion bit and another base yields the insertion only
    when its base is the reference's"""
    out = {}
    for t, d, c, ins, ref, call in variants:
        if call & 15 == R.DEL:
            out[t] = ("del", "")
        elif call & 15 != ref:
            out[t] = ("sub", "ACGT"[call & 15])
        if call & R.INS_BIT:
            assert t not in out
            out[t] = ("ins", voted[t][0])
    return out


def test_end_to_end_planted_edits(api):
    strs, copies, reads, planted = planted_case(E2E_SEED)
    fm = index_of(api, strs)
    mp = fm.map(reads)
    res = mp.pileup(fm, reads, min_mapq=20)
    cr = res.call()
    voted = {t: (s, sup, d) for t, s, sup, d in cr.insertions()}
    assert found_set(var_tuples(cr.variants), voted) == planted
    cons = dict(cr.consensus())
    for r, c in enumerate(copies):
        assert cons[r].upper() == c, r
    # and the device agrees with the definition on these alignments
    alns, cigars = unpack(mp.alignments(20))
    table, calls, variants, rvoted, rcons = R.run(reads, alns, cigars, strs)
    assert np.array_equal(res.counts, np.array(table, dtype=np.uint32))
    assert cr.calls.tolist() == calls and var_tuples(cr.variants) == variants and voted == rvoted
    assert [cons[r] for r in range(3)] == rcons
    fm.close()
