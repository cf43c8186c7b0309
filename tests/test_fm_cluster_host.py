"""Seed clustering of the read mapper (debwt_fm_cluster_seeds): pure host code, driven on hand-made seeds without a GPU.
Seeds are (strand, record, diag, qbeg, qend); a candidate is (strand, record, diag, first_diag, weight, seeds)."""
import pytest


@pytest.fixture(scope="module")
def cluster():
    from debwt_amd import api
    return api.cluster_seeds


def keys(cands, *names):
    return [tuple(c[n] for n in names) for c in cands]


def test_empty_and_single(cluster):
    assert cluster([]) == []
    c = cluster([(0, 2, 1000, 5, 30)])
    assert c == [{"diag": 1000, "first_diag": 1000, "record": 2, "strand": 0, "weight": 25, "seeds": 1}]


def test_band_boundary(cluster):
    # within w of the cluster's FIRST seed joins, w + 1 opens a new cluster; the anchor does not move with later seeds
    seeds = [(0, 0, 100, 0, 20), (0, 0, 116, 30, 50), (0, 0, 117, 60, 80), (0, 0, 132, 85, 99)]
    c = cluster(seeds, band=16)
    assert sorted(keys(c, "first_diag", "seeds", "weight")) == [(100, 2, 40), (117, 2, 34)]
    c = cluster(seeds, band=17)
    assert sorted(keys(c, "first_diag", "seeds")) == [(100, 3), (132, 1)]
    assert sorted(keys(cluster(seeds, band=0), "first_diag")) == [(100,), (116,), (117,), (132,)]
    # negative diagonals (a read hanging over the start of the text) sort and cluster like any other
    c = cluster([(0, 0, -5, 5, 30), (0, 0, 3, 40, 60), (0, 0, 12, 70, 90)], band=16)
    assert keys(c, "first_diag", "seeds") == [(-5, 2), (12, 1)]


def test_weight_is_distinct_query_positions(cluster):
    # overlapping and nested seeds count every query position once
    c = cluster([(1, 0, 50, 0, 30), (1, 0, 50, 10, 40), (1, 0, 52, 12, 20), (1, 0, 51, 60, 70)])
    assert keys(c, "weight", "seeds") == [(50, 4)]


def test_diag_of_longest_seed(cluster):
    c = cluster([(0, 0, 200, 50, 70), (0, 0, 203, 0, 31), (0, 0, 206, 72, 100)])
    assert keys(c, "diag", "first_diag") == [(203, 200)]
    # ties in length: the smallest qbeg; then the smallest diag
    c = cluster([(0, 0, 205, 40, 60), (0, 0, 201, 10, 30), (0, 0, 209, 70, 90)])
    assert keys(c, "diag") == [(201,)]
    c = cluster([(0, 0, 207, 10, 30), (0, 0, 202, 10, 30)])
    assert keys(c, "diag") == [(202,)]


def test_records_and_strands_never_mix(cluster):
    seeds = [(0, 0, 100, 0, 20), (0, 1, 100, 0, 25), (1, 0, 100, 0, 30), (1, 1, 101, 0, 35), (1, 1, 100, 40, 50)]
    c = cluster(seeds)
    assert keys(c, "strand", "record", "weight", "seeds") == [(1, 1, 45, 2), (1, 0, 30, 1), (0, 1, 25, 1), (0, 0, 20, 1)]


def test_order_ties_and_max_cand(cluster):
    # equal weights: smaller (strand, record, first diag) first
    seeds = [(1, 0, 10, 0, 20), (0, 1, 500, 0, 20), (0, 1, 100, 0, 20), (0, 0, 900, 0, 20), (0, 0, 40, 5, 30)]
    c = cluster(seeds, band=16, max_cand=8)
    assert keys(c, "strand", "record", "first_diag") == [(0, 0, 40), (0, 0, 900), (0, 1, 100), (0, 1, 500), (1, 0, 10)]
    assert keys(cluster(seeds, max_cand=2), "strand", "record", "first_diag") == [(0, 0, 40), (0, 0, 900)]
    assert cluster(seeds, max_cand=0) == []
    # input order does not matter
    assert cluster(list(reversed(seeds))) == c


def test_empty_seed_is_refused(cluster):
    from debwt_amd import api
    with pytest.raises(api.DebwtError) as e:
        cluster([(0, 0, 5, 10, 10)])
    assert e.value.code == -1
