"""The texts of tests/k_ladder.py do what tests/test_k_sweep_gpu.py relies on -- shown on the reference side alone (the
oracle and numpy, no GPU): the result does not depend on k, the intermediates do at EVERY step of k, and the definition of
the keys used there is the oracle's."""
import numpy as np
import pytest

import k_ladder as KL

TEXTS = ("small", "mid")


@pytest.fixture(scope="module")
def exp(oracle):
    return {name: KL.expected(name) for name in TEXTS}


def test_shape_of_the_texts():
    for name in TEXTS:
        assert all(len(r) > 32 for r in KL.records(name))
    assert 8_000 < KL.n_symbols("small") < 12_000
    assert 90_000 < KL.n_symbols("mid") <= 100_000
    assert len(KL.records("mid")) == len(KL.records("small")) + 3


@pytest.mark.parametrize("name", TEXTS)
def test_bwt_does_not_depend_on_k(exp, name):
    assert exp[name].k_invariant


def test_small_equals_the_definition(oracle, exp):
    assert np.array_equal(exp["small"].rows, oracle.naive_bwt(exp["small"].sym))


@pytest.mark.parametrize("name", TEXTS)
def test_counters_move_with_k(exp, name):
    E = exp[name]
    assert all(E.stats[k]["special_branch_num"] > 0 for k in KL.KS), [E.stats[k]["special_branch_num"] for k in KL.KS]
    caps = [E.stats[k]["red_capacity"] for k in KL.KS]
    assert len(set(caps)) >= 18, caps


@pytest.mark.parametrize("name", TEXTS)
@pytest.mark.parametrize("k", KL.KS[:-1])
def test_a_neighbouring_k_gives_other_intermediates(exp, name, k):
    """the red array or the SP symbols at k differ from those at k + 1: a kernel that used K + 1 or K - 1 fails the
    stage comparisons"""
    E = exp[name]
    assert not (np.array_equal(E.red[k], E.red[k + 1]) and np.array_equal(E.sp[k], E.sp[k + 1]))


@pytest.mark.parametrize("name", TEXTS)
@pytest.mark.parametrize("k", KL.KS)
def test_key_definition_is_the_oracles(oracle, exp, name, k):
    """oracle.kmer_count counts the k-mers (k symbols, left-aligned: src/mySort.c:193-195), a key holds a node of
    K = k - 1 symbols and the symbol in front of it: every k-mer of a record is (pred, node) of one of its keys but the
    first, whose pred is the separator's.  Both fields of the definition are tied to the oracle that way."""
    recs = KL.records(name)
    keys = KL.node_keys(recs, k)
    K = k - 1
    first = np.zeros(len(keys), dtype=bool)
    first[np.cumsum([0] + [len(r) - K + 1 for r in recs[:-1]])] = True
    assert (keys[first] & np.uint64(3) == 3).all()
    inner = keys[~first]
    kmers = ((inner & np.uint64(3)) << np.uint64(2 * K)) | (inner >> np.uint64(2))
    km, counts = np.unique(kmers << np.uint64(64 - 2 * k), return_counts=True)
    okm, oct_ = oracle.kmer_count(exp[name].sym, k)
    assert np.array_equal(km, okm) and np.array_equal(counts.astype(np.uint64), oct_)


def test_mid_is_above_the_two_digit_threshold():
    assert len(KL.node_keys(KL.records("mid"), 32)) > 1 << 14
