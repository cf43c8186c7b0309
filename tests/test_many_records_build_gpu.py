"""The builder, the verifier and an index made by the builder at 2^24 + 512 records.  The records are 63 random bases each
(two packed words with the separator on the last position), so the collection is made in a second; about 4,096 records
are overwritten with copies of others, so duplicate records exist with known multiplicity, and the first words prove
every other record distinct.  The suffixes that begin with '#' are the last nrec rows: none of them holds a separator and
every line there has all nrec - 1 '#' rows before it, so the verifier's v_occ reads 'T' counts through the high half of
the separators-before count on more than 4 * 10^4 lines, and the special-region module of the builder runs on the device
with more than 1.6 * 10^7 records.  tests/test_fm_many_records_gpu.py covers the queries on an index with lines of that
kind among the base suffixes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HIGH = 1 << 24
R = HIGH + 512
ROWS = 384
N = 64 * R


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def collection():
    """(words, sep, groups): the packed text as api.pack_records documents it, the separator positions, and per planted
    string the records that hold it (the source first)"""
    rng = np.random.default_rng(2024)
    w = rng.integers(0, 2 ** 64, size=(R, 2), dtype=np.uint64)
    w[:, 1] |= np.uint64(3)                                              # position 63 of every record: the separator, as 'T'
    pick = rng.choice(np.arange(1, HIGH - 64), 2048 + 4096 - 8, replace=False)
    src, t1, t2, t3 = pick[:2048], pick[2048:4096 - 8], pick[4088:5112], pick[5112:6136]
    t1 = np.concatenate([HIGH + 1 + 5 * np.arange(8), t1])               # eight copies stand behind record 2^24
    w[t1] = w[src]
    w[t2] = w[src[:1024]]
    w[t3] = w[src[:1024]]
    groups = [[int(src[j]), int(t1[j])] + ([int(t2[j]), int(t3[j])] if j < 1024 else []) for j in range(2048)]
    first, counts = np.unique(w[:, 0], return_counts=True)
    assert len(first) == R - 4096                                       # every record that was not overwritten is distinct
    assert np.count_nonzero(counts == 2) == 1024 and np.count_nonzero(counts == 4) == 1024
    words = np.concatenate([w.reshape(-1), np.array([2 ** 64 - 1, 0], dtype=np.uint64)])   # 32 'T' of padding, zeros
    sep = np.arange(R, dtype=np.uint64) * np.uint64(64) + np.uint64(63)
    return words, sep, groups


def code_census(words):
    """2-bit codes of packed words, by value"""
    per_byte = np.bincount(words.view(np.uint8), minlength=256).astype(np.int64)
    v = np.arange(256)
    return np.array([sum(int(per_byte[(v >> s) & 3 == c].sum()) for s in (0, 2, 4, 6)) for c in range(4)], dtype=np.int64)


def record_bytes(words, rec):
    """the 63 bases of the given records as ASCII"""
    w = words[:2 * R].reshape(R, 2)[np.asarray(rec)]
    shift = (2 * (31 - np.arange(32))).astype(np.uint64)
    codes = ((w[:, :, None] >> shift[None, None, :]) & np.uint64(3)).reshape(len(w), 64)[:, :63]
    return [bytes(r) for r in np.frombuffer(b"ACGT", dtype=np.uint8)[codes]]


def test_build_verify_and_query_at_2_24_records(api):
    import torch
    words, sep, groups = collection()
    d = api.DeBWT(k=32)
    d.load_packed(words, N, sep)

    # 1. build
    d.build()
    st = d.stats()
    assert st["nrec"] == R and st["special_path"] == 2, st
    assert np.array_equal(d.bwt_census().astype(np.int64), code_census(words[:2 * R]))
    rows, hrows, drow = d.fetch()
    assert len(hrows) == R - 1 and bool((np.diff(hrows.astype(np.int64)) > 0).all())
    assert int(hrows[-1]) < N - R                                       # no '#' row among the '#' suffixes

    # 2. verify: the built rows, then the same rows with two unequal rows swapped inside a line of the '#' suffixes,
    #    one of them a 'T' row -- 2^24 + 511 separator rows stand before that line and none in it
    assert d.verify_device()["inverse_bwt_ok"]
    code = lambda a, r: int(a[r >> 5] >> np.uint64(2 * (31 - (r & 31)))) & 3       # noqa: E731
    line = (N - R // 2) // ROWS
    at = [line * ROWS + j for j in range(ROWS)]
    i = next(r for r in at if code(rows, r) == 3)
    j = next(r for r in at if code(rows, r) != 3)
    assert drow not in (i, j) and hrows[-1] < min(i, j)
    bad = rows.copy()
    for pos, s in ((i, code(rows, j)), (j, 3)):
        sh = np.uint64(2 * (31 - (pos & 31)))
        bad[pos >> 5] = (bad[pos >> 5] & ~(np.uint64(3) << sh)) | (np.uint64(s) << sh)
    good_dev = torch.from_numpy(rows.view(np.int64)).cuda()
    assert d.verify_device(good_dev.data_ptr(), hrows, drow)["inverse_bwt_ok"]
    bad_dev = torch.from_numpy(bad.view(np.int64)).cuda()
    assert not d.verify_device(bad_dev.data_ptr(), hrows, drow)["inverse_bwt_ok"]
    del good_dev, bad_dev

    # 3. query: whole records as patterns
    fm = d.fm_index(sa_sample=32)
    plain = [0, 1, R - 2, R - 1] + list(range(HIGH - 6, HIGH + 7))      # copies of nothing
    plain = [r for r in plain if all(r not in g for g in groups)]
    rng = np.random.default_rng(7)
    others = rng.choice(np.arange(8, 2048), 2000 - 8 - len(plain), replace=False)
    chosen = [groups[j] for j in range(8)] + [groups[int(j)] for j in others]
    want = chosen + [[r] for r in plain]
    pats = record_bytes(words, [g[0] for g in want])
    assert len(pats) == 2000 and len(pats[0]) == 63 and max(max(g) for g in want) > HIGH
    assert fm.count(pats).tolist() == [len(g) for g in want]
    where = fm.locate(pats)
    for g, pos in zip(want, where):
        assert sorted(pos.tolist()) == [64 * r for r in sorted(g)], g
        rec, off = fm.resolve(pos)
        assert sorted(rec.tolist()) == sorted(g) and not off.any()
    every = sorted({r for g in want for r in g})
    got = fm.extract([(r,) for r in every])
    assert got == record_bytes(words, every)
    fm.close()
    d.close()
