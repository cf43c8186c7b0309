"""many_records_ref on the CPU: the closed-form index equals the sorted one where sorting is affordable, the large
instance holds the rank lines it is built for, and the patterns of test_fm_many_records_gpu.py would give another answer
if any of the three decoders of a line's separators-before count lost its high 24 bits.

The groups of test_patterns_need_the_high_bits and the decoder each pins on the GPU:
    one    a 'T' step with lo and hi in one header-branch line    fm_occ2        ranges, count, locate, mems, overlaps
    two    a 'T' step with lo and hi in two lines                 v_occ          ranges, count, locate
    four   a step that reads all four codes of a line             fm_line_occ4   search, k-mer table, spectrum, overlaps_mm
    head   LF from a 'T' row among the head's suffixes            v_occ (v_lf)   locate walks, extract, restore_text, esa
    tail   LF from a 'T' row among the last '#' suffixes          v_occ (v_lf)   locate walks, restore_text, esa

The whole file takes about 18 s, nearly all of it the large instance (index, model and Esa), which is made once."""
import numpy as np
import pytest

import esa_ref
import fm_definition as F
import many_records_ref as M


@pytest.mark.parametrize("lens", [(300, 250, 200), M.HEAD_LENS])
@pytest.mark.parametrize("NA,NT", [(1, 1), (2, 1), (1, 3), (5, 4), (40, 50), (400, 50)])
def test_analytic_index_is_the_definition(lens, NA, NT):
    recs = M.head(M.SEED, lens)
    X = M.Index(recs, NA, NT)
    sym, sa, L, words, hash_rows, dollar_row = F.definition_index(list(recs) + [M.A1] * NA + [M.T1] * NT)
    assert np.array_equal(X.sym, sym) and np.array_equal(X.sa, sa) and np.array_equal(X.L, L)
    assert np.array_equal(X.words, words) and np.array_equal(X.hash_rows, hash_rows) and X.dollar_row == dollar_row
    assert X.nrec == 3 + NA + NT
    want = F.line_profile(L)
    got = M.line_profile(L)
    assert [tuple(int(v[b]) for v in got) for b in range(len(want))] == want


def test_guard_refuses_a_head_whose_order_does_not_carry_over():
    """GC # ATC # GC: the suffixes C#ATC.. and C#A#.. are told apart behind the first 'A' record only.  A head over
    {C, G, T} cannot do that (it holds no "#A" but at its end), which analytic_index asserts by the alphabet."""
    recs = tuple(np.array(r, dtype=np.uint8) for r in ([2, 1], [0, 3, 1], [2, 1]))
    with pytest.raises(AssertionError, match="told apart"):
        M.head_order(recs)
    with pytest.raises(AssertionError):
        M.analytic_index(recs, 2, 2)


def test_scaled_instance_and_intervals():
    D, X = M.scaled(), M.index(*M.SCALED)
    assert D.nrec == X.nrec == 3 + sum(M.SCALED)
    for p in M.range_patterns()[::7] + tuple(w.encode() for w in M.SHORT_PATTERNS):
        assert X.interval(p) == D.interval(p), p
    E, S = M.esa(*M.SCALED), esa_ref.Esa(D.records, D.sa)
    assert np.array_equal(E.da, S.da) and np.array_equal(E.lcp_full, S.lcp_full) and E.summary() == S.summary()
    assert E.profile(16) == S.profile(16)


def test_full_size_facts():
    X = M.index()
    NA, NT = M.FULL
    assert NA > M.HIGH and X.nrec == 3 + NA + NT and X.n == X.H + 2 * (NA + NT)
    assert X.n % M.ROWS and X.n % 32                                   # a partial last line and a partial last word
    head, tail = X.high_lines(X.head_rows), X.high_lines(X.tail_rows)
    assert len(head) >= 4 and len(tail) >= 4, (len(head), len(tail))
    assert len(X.high_lines()) == len(head) + len(tail)
    # direct counts
    assert X.dollar_row == int(np.nonzero(X.sa == 0)[0][0])
    assert len(X.hash_rows) == X.nrec - 1
    assert np.array_equal(X.hash_rows, np.nonzero(X.sym[X.sa - 1] == F.SEP)[0])
    text = np.bincount(X.sym, minlength=6)
    assert X.census().tolist() == [text[0], text[1], text[2], text[3] + text[4] + text[5]]
    assert text[0] == NA and text[4] == X.nrec - 1 and text[5] == 1
    assert int(X.before[-1] + X.seps[-1]) == X.nrec
    # the suffix array is one: a permutation whose neighbours ascend, checked on the seams of the construction and on
    # sampled rows (the blocks between are arithmetic progressions of equal suffixes up to their length)
    seen = np.zeros(X.n, dtype=bool)
    seen[X.sa] = True
    assert seen.all()
    b = X._bytes
    rng = np.random.default_rng(5)
    seams = np.cumsum([NA, X.H - 3, NT, 1, NA - 1, 2, 1, NT - 1])
    rows = np.unique(np.concatenate([seams - 1, seams, seams + 1, rng.integers(1, X.n, 100)]))
    for r in rows[(rows > 0) & (rows < X.n)].tolist():
        assert b[int(X.sa[r - 1]):] < b[int(X.sa[r]):], r
    for r in range(X.head_rows[0] + 1, X.head_rows[1]):                # decided inside the head (head_order's guard)
        assert b[int(X.sa[r - 1]):X.H] < b[int(X.sa[r]):X.H], r


def test_full_size_esa_facts():
    E, X = M.esa(), M.index()
    NA, NT = M.FULL
    assert E.records is None and E.n == X.n
    assert int(E.da.max()) == X.nrec - 1 > M.HIGH
    assert np.array_equal(E.da[:NA], 3 + np.arange(NA))                 # the A# rows: record numbers past 2^24
    assert (E.lcp_full[1:NA] == 1).all() and E.lcp_full[0] == 0
    assert E.profile(2)[0] == 4                                         # A, C, G, T


def groups():
    """group -> [(what, answer of the model, answer of the model without the high bits, the reference)]"""
    X, R = M.index(), M.model()
    out = {"one": [], "two": [], "four": [], "head": [], "tail": []}
    for p in M.range_patterns():
        got, kinds = R.backward(p)
        for kind in kinds:
            out[kind].append((p, got, R.backward(p, drop_high=True)[0], X.interval(p)))
    for p in [r.upper() for r in M.reads() if "N" not in r.upper()] + [w.decode().upper() for w in M.locate_patterns()[:40]]:
        got, kinds = R.backward(p, four=True)
        if kinds:
            out["four"].append((p, got, R.backward(p, drop_high=True, four=True)[0], X.interval(p)))
    head_rows = []
    for p in M.locate_patterns():
        lo, hi = X.interval(p)
        head_rows += [r for r in range(lo, hi) if X.L[r] == 3 and r // M.ROWS in R._high()]
    isa_of = lambda r: (int(X.sa[r]) - 1) % X.n                                      # noqa: E731
    for name, rows in (("head", head_rows), ("tail", M.tail_t_rows(X).tolist())):
        for r in rows:
            nr, s = R.lf(r)
            assert s == 3 and int(X.sa[nr]) == isa_of(r), r                          # the model's LF is the definition's
            out[name].append((r, nr, R.lf(r, drop_high=True)[0], nr))
    return out


def test_patterns_need_the_high_bits():
    for name, rows in groups().items():
        assert rows, name
        differ = 0
        for what, got, dropped, want in rows:
            if name in ("head", "tail") or want[1] > want[0]:
                assert got == want, (name, what, got, want)
            else:                                                       # no occurrence: lo is no function of the pattern
                assert got[0] == got[1], (name, what, got, want)
            differ += dropped != got
        assert differ >= 1, name
        if name in ("head", "tail"):
            assert differ == len(rows), name


def test_model_is_the_definition_where_nothing_is_dropped():
    """occ of the model against direct counts over L, at rows of every kind of line"""
    X, R = M.index(), M.model()
    rng = np.random.default_rng(6)
    lines = np.concatenate([X.high_lines(), rng.integers(0, len(X.seps), 40), [0, len(X.seps) - 1]])
    cum = {s: None for s in range(4)}
    for s in range(4):
        cum[s] = np.concatenate([[0], np.cumsum(X.L == s, dtype=np.int32)])
    for b in lines.tolist():
        for i in {b * M.ROWS, min(b * M.ROWS + int(rng.integers(0, M.ROWS)), X.n), min((b + 1) * M.ROWS - 1, X.n)}:
            want = [int(cum[s][i]) for s in range(4)]
            assert [R.occ(s, i) for s in range(4)] == want and R.occ4(i) == want, i
