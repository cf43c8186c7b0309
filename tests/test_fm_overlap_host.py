"""debwt_fm_overlap_longest (api.overlap_longest), the host reduction behind DEBWT_FM_OVERLAP_LONGEST, without a GPU:
against a literal Python reduction on random hit lists in the documented order, idempotent, and DEBWT_EINVAL for every
way of breaking that order."""
import numpy as np
import pytest

from overlap_ref import longest_of


@pytest.fixture(scope="module")
def api():
    from debwt_amd import api as A
    return A


def random_lists(rng, npat):
    """per pattern a list of (record, length, strand, flags) by (strand, length descending, record ascending): few records
    and few lengths, so records repeat at several lengths; some patterns empty, some with one strand only"""
    out = []
    for _ in range(npat):
        hits = []
        kind = int(rng.integers(0, 5))
        for strand in (0, 1):
            if kind == 0 or (kind == 1 and strand == 0) or (kind == 2 and strand == 1):
                continue
            for L in sorted({int(x) for x in rng.integers(1, 40, int(rng.integers(1, 9)))}, reverse=True):
                for rec in sorted({int(x) for x in rng.integers(0, 12, int(rng.integers(1, 8)))}):
                    hits.append((rec, L, strand, int(rng.integers(0, 4))))
        out.append(hits)
    return out


def arrays(api, lists):
    offs = np.zeros(len(lists) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in lists], out=offs[1:])
    flat = [h for x in lists for h in x]
    return np.array(flat, dtype=api._OVERLAP_DTYPE) if flat else np.zeros(0, dtype=api._OVERLAP_DTYPE), offs


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_against_python_reduction(api, seed):
    rng = np.random.default_rng(seed)
    lists = random_lists(rng, 60)
    assert any(not x for x in lists) and any(len({(h[0], h[2]) for h in x}) < len(x) for x in lists)
    hits, offs = arrays(api, lists)
    got, goffs = api.overlap_longest(hits, offs)
    want, woffs = arrays(api, [longest_of(x) for x in lists])
    assert np.array_equal(goffs, woffs)
    assert np.array_equal(got, want)
    assert len(got) < len(hits)
    again, aoffs = api.overlap_longest(got, goffs)            # idempotent
    assert np.array_equal(again, got) and np.array_equal(aoffs, goffs)
    assert np.array_equal(hits, arrays(api, lists)[0])        # the caller's array is not touched


def test_long_strand_segments(api):
    """hundreds of hits of one pattern and strand (a low-complexity read): the path past the small-segment scan"""
    rng = np.random.default_rng(9)
    lists = []
    for _ in range(4):
        hits = []
        for strand in (0, 1):
            for L in range(90, 20, -1):
                for rec in sorted({int(x) for x in rng.integers(0, 40, 12)}):
                    hits.append((rec, L, strand, 0))
        lists.append(hits)
    assert min(len(x) for x in lists) > 1000
    hits, offs = arrays(api, lists)
    got, goffs = api.overlap_longest(hits, offs)
    want, woffs = arrays(api, [longest_of(x) for x in lists])
    assert np.array_equal(goffs, woffs) and np.array_equal(got, want)


def test_empty(api):
    got, offs = api.overlap_longest(np.zeros(0, dtype=api._OVERLAP_DTYPE), [0])
    assert len(got) == 0 and offs.tolist() == [0]
    got, offs = api.overlap_longest(np.zeros(0, dtype=api._OVERLAP_DTYPE), [0, 0, 0])
    assert len(got) == 0 and offs.tolist() == [0, 0, 0]


def test_rejects_broken_order(api):
    ok = [[(1, 30, 0, 0), (4, 30, 0, 0), (1, 20, 0, 0), (2, 25, 1, 0)], [(0, 9, 1, 0)]]
    hits, offs = arrays(api, ok)
    api.overlap_longest(hits, offs)
    broken = {
        "length ascending": [[(1, 20, 0, 0), (1, 30, 0, 0)]],
        "records descending in one length": [[(4, 30, 0, 0), (1, 30, 0, 0)]],
        "a record twice in one length": [[(4, 30, 0, 0), (4, 30, 0, 0)]],
        "strand descending": [[(1, 30, 1, 0), (1, 30, 0, 0)]],
        "strand above 1": [[(1, 30, 2, 0)]],
        "second pattern broken": [[(1, 30, 0, 0)], [(1, 5, 0, 0), (1, 6, 0, 0)]],
    }
    for why, lists in broken.items():
        h, o = arrays(api, lists)
        with pytest.raises(api.DebwtError) as e:
            api.overlap_longest(h, o)
        assert e.value.code == -1, why
    with pytest.raises(api.DebwtError) as e:                  # decreasing offsets
        api.overlap_longest(hits, np.array([0, 4, 3, 5], dtype=np.uint64))
    assert e.value.code == -1
    # an order that only holds across a pattern boundary is fine: every pattern is checked on its own
    h, o = arrays(api, [[(1, 5, 1, 0)], [(1, 30, 0, 0)]])
    got, _ = api.overlap_longest(h, o)
    assert len(got) == 2
