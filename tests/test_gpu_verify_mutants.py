"""The refusing side of the inverse-BWT verifiers on the GPU: every near-miss of the true rows that
tests/verify_mutants.py enumerates (a few thousand per collection, 11 collections) goes through debwt_verify_device at
segments 0, 1, 7 and 64, a sample of 400 per collection through debwt_fm_create, the malformed ones through
debwt_fm_open, and the true rows of every mutated text through debwt_verify_device.  The verdict needs no tolerance: the
true rows are accepted with the segment count verify_mutants.expected_segments restates, everything else is refused --
as a bad input (DEBWT_EINVAL with a reason) where verify_mutants.guard_applies says so, by the walk otherwise.  Which
counter refuses is not pinned for every mutant, but one refused mutant in 16 has all six counters of its report compared
with verify_mutants.segmented_report, the walk restated in Python.
tests/test_verify_mutants_ref.py holds the mutants, the reference verdict, guard_applies and segmented_report to account
on the CPU; its test_the_segmented_walk_refuses_what_the_reference_refuses says why no mutant is refused by a broken link
alone, so that a verdict that ignored broken_links would pass here (tried: it does).

No input here can take an LF step outside [0, n).  The library refuses, on the host or by a count over the listed rows
before any search or walk: a list entry >= n, '#' rows that do not strictly ascend, the '$' row among the '#' rows, a
listed row whose code is not 3 (classes E and F, part of C3 and D).  For all that is left (A, B, C1, C2, P, T, the rest
of C3 and D):
  - C[] is taken from the mutated rows' own census, so C[s] + occ(s, i) <= C[s] + tot[s] = C[s + 1] <= n for a base s,
    and < C[s + 1] when row i itself holds s, which is the case in every LF step;
  - every listed row holds code 3, so occ('T', i) = code-3 rows before i minus listed rows before i is never negative,
    and C['T'] + occ('T', i) <= C['T'] + tot[3] - nrec = C['#'];
  - the lists are strictly ascending and distinct, so the j-th '#' row maps to C['#'] + j <= n - 2 and the '$' row to
    n - 1.
The walks are bounded by the text length and the searches by maxm, whatever the rows hold.

The words of a case live in one device tensor; a mutant is made by writing its one or two changed words and undone
afterwards, so the tensor is uploaded once per test.  All classes are complete on every case (STRIDE = 1: nothing is
thinned: the slowest test takes 2.4 s; profiles/r29_verify_mutants.txt has the wall time and the mutant count of every
test)."""
import collections
import contextlib
import time

import numpy as np
import pytest

import fm_definition as F
import verify_mutants as M

pytestmark = pytest.mark.gpu
SEGMENTS = (0, 1, 7, 64)
EINVAL = -1
STRIDE = 1                       # of classes A and B on the cases with n > 768, were they thinned: they are not
TEXT_CASES = ("n383", "n384", "n385", "all_T_400_37_33")
FM_MUTANTS = 400
REPORT_STRIDE = 16               # one refused mutant in 16 has every counter of its report compared, not only the verdict
REASON = {"E": ("code other than 3",), "F": ("'$' row outside", "'#' rows are not ascending")}

every_case = pytest.mark.parametrize("name", M.CASE_NAMES)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def thinned(name):
    """the mutants of a case: all of them, but every STRIDE-th of classes A and B where n > 768"""
    D, seen = M.case(name), collections.Counter()
    for m in M.mutant_list(name):
        seen[m[0]] += 1
        if STRIDE > 1 and D.n > 768 and m[0][0] in "AB" and (seen[m[0]] - 1) % STRIDE:
            continue
        yield m


class DeviceRows:
    """the true words of a case in one device tensor"""

    def __init__(self, D):
        import torch
        self.torch, self.words, self.clean = torch, D.words, D.words.view(np.int64)
        self.t = torch.from_numpy(self.clean.copy()).cuda()
        self.ptr = self.t.data_ptr()
        torch.cuda.synchronize()

    @contextlib.contextmanager
    def holding(self, words):
        """the tensor holds `words` inside the block: the changed words written, then written back"""
        w = words.view(np.int64)
        idx = [] if words is self.words else np.nonzero(w != self.clean)[0].tolist()
        assert len(idx) <= 2
        try:
            for i in idx:
                self.t[i] = int(w[i])
            if idx:
                self.torch.cuda.synchronize()                   # the library reads on a stream of its own
            yield
        finally:
            for i in idx:
                self.t[i] = int(self.clean[i])
            if idx:
                self.torch.cuda.synchronize()

    def is_clean(self):
        return np.array_equal(self.t.cpu().numpy(), self.clean)


def check_accepted(r, D, segments):
    rep = r["inverse_bwt"]
    assert r["inverse_bwt_ok"], r
    assert rep["steps"] == D.n - 1 and rep["mismatches"] == 0 and rep["broken_links"] == 0 and rep["search_failures"] == 0, r
    assert rep["segments"] == M.expected_segments(D.sym, D.sa, D.n, segments), r
    assert rep["search_steps"] == M.segmented_report(D.words, D.n, D.hash_rows, D.dollar_row, D.sym, segments)["search_steps"]


def check_refused_input(api, cls, call):
    with pytest.raises(api.DebwtError) as e:
        call()
    assert e.value.code == EINVAL, (cls, str(e.value))
    if cls in REASON:
        assert any(why in str(e.value) for why in REASON[cls]), (cls, str(e.value))


# ---- debwt_verify_device -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("segments", SEGMENTS)
@every_case
def test_verify_device_accepts_the_rows_and_refuses_every_mutant(api, name, segments):
    D = M.case(name)
    d = api.DeBWT(k=32)                                         # k = 32: recs_30x33 only just has n > nrec * 32
    d.load_records(D.records)
    rows = DeviceRows(D)
    t0 = time.perf_counter()
    check_accepted(d.verify_device(rows.ptr, D.hash_rows, D.dollar_row, segments=segments), D, segments)
    count = collections.Counter()
    for i, (cls, words, hrows, drow) in enumerate(thinned(name)):
        count[cls] += 1
        with rows.holding(words):
            call = lambda: d.verify_device(rows.ptr, hrows, drow, segments=segments)          # noqa: E731
            if cls == "P":
                check_accepted(call(), D, segments)
            elif M.guard_applies(D, cls, words, hrows, drow):
                check_refused_input(api, cls, call)
            else:
                r = call()
                assert not r["inverse_bwt_ok"], (cls, i, drow, r)
                if i % REPORT_STRIDE == 0:                      # every counter against the restated walk
                    want = M.segmented_report(words, D.n, hrows, drow, D.sym, segments)
                    assert {k: r["inverse_bwt"][k] for k in want} == want, (cls, i, drow)
    assert rows.is_clean()
    check_accepted(d.verify_device(rows.ptr, D.hash_rows, D.dollar_row, segments=segments), D, segments)   # no state kept
    print(f"\n{name} segments={segments}: {sum(count.values())} mutants in {time.perf_counter() - t0:.2f} s {dict(count)}")
    d.close()


@pytest.mark.parametrize("name", TEXT_CASES)
def test_verify_device_refuses_the_rows_on_every_mutated_text(api, name):
    D = M.case(name)
    d = api.DeBWT(k=32)
    rows = DeviceRows(D)
    t0, texts = time.perf_counter(), 0
    for cls, recs in M.text_mutants(D.records):
        d.load_records(recs)
        texts += 1
        for segments in (0, 64):
            r = d.verify_device(rows.ptr, D.hash_rows, D.dollar_row, segments=segments)
            assert not r["inverse_bwt_ok"], (texts, segments, r)
    d.load_records(D.records)
    for segments in (0, 64):
        check_accepted(d.verify_device(rows.ptr, D.hash_rows, D.dollar_row, segments=segments), D, segments)
    print(f"\n{name}: {texts} texts at 2 settings in {time.perf_counter() - t0:.2f} s")
    d.close()


# ---- debwt_fm_create and debwt_fm_open ---------------------------------------------------------------------------------

def fm_sample(name):
    """at most FM_MUTANTS mutants: all of C1, C2, E and F and a seeded sample of the rest; P apart"""
    every = [m for m in M.mutant_list(name) if m[0] != "P"]
    keep = [m for m in every if m[0] in ("C1", "C2", "E", "F")]
    rest = [m for m in every if m[0] not in ("C1", "C2", "E", "F")]
    rng = np.random.default_rng(len(every))
    pick = sorted(rng.choice(len(rest), size=min(len(rest), FM_MUTANTS - len(keep)), replace=False).tolist())
    assert len(keep) < FM_MUTANTS // 2
    return keep + [rest[i] for i in pick], [m for m in M.mutant_list(name) if m[0] == "P"]


def count_patterns(D):
    pats = [a + b + c for a in [""] + list(F.ACGT) for b in [""] + list(F.ACGT) for c in F.ACGT]
    return sorted(set(pats)) + [s[:m] for s in D.strs[:3] for m in (7, 20, 33)]


@every_case
def test_fm_create_refuses_the_mutants(api, name):
    D = M.case(name)
    d = api.DeBWT(k=32)
    d.load_records(D.records)
    bad, padded = fm_sample(name)
    assert len(bad) <= FM_MUTANTS and {m[0] for m in bad} >= {"A", "D", "E", "F"}
    t0 = time.perf_counter()
    for cls, words, hrows, drow in bad:
        check_refused_input(api, cls, lambda: d.fm_index(rows=(words, hrows, drow)))
    took = time.perf_counter() - t0
    pats = count_patterns(D)
    for s in (1, 32):
        fm = d.fm_index(sa_sample=s, rows=(D.words, D.hash_rows, D.dollar_row))
        assert np.array_equal(fm.samples(), D.sa[::s].astype(np.uint64)), s
        census, counts = fm.info()["census"], fm.count(pats)
        fm.close()
    assert np.array_equal(census, D.census())
    assert np.array_equal(counts, [D.interval(p)[1] - D.interval(p)[0] for p in pats])
    for cls, words, hrows, drow in padded:
        fm = d.fm_index(rows=(words, hrows, drow))
        assert np.array_equal(fm.info()["census"], census) and np.array_equal(fm.count(pats), counts)
        assert np.array_equal(fm.samples(), D.sa[::32].astype(np.uint64))
        fm.close()
    print(f"\n{name}: {len(bad)} mutants refused by debwt_fm_create in {took:.2f} s")
    d.close()


@every_case
def test_fm_open_refuses_bad_lists_and_codes(api, name):
    D = M.case(name)
    samples = F.samples(D.sa, 32)
    seen = 0
    for cls, words, hrows, drow in M.mutant_list(name):
        if cls in ("E", "F"):
            with pytest.raises(api.DebwtError) as e:
                api.FMIndex.open(words, D.n, hrows, drow, samples, sa_sample=32)
            assert e.value.code == EINVAL, (cls, seen)
            seen += 1
    assert seen >= 6
    fm = api.FMIndex.open(D.words, D.n, D.hash_rows, D.dollar_row, samples, sa_sample=32)
    assert np.array_equal(fm.info()["census"], D.census())
    fm.close()
