"""Extract and text restore (debwt_fm_extract, debwt_fm_restore_text, debwt_fm_text_fetch) on indexes opened from rows
and samples alone -- no text is anywhere near the index under test.  The expected strings are the golden records; the
rows are the golden OUT / OUT.# / OUT.$ files (for the goldens kept as hashes: a build whose hashes match); the samples
come from an index made by debwt_fm_create and read out with samples()."""
import ctypes
import hashlib

import numpy as np
import pytest

from conftest import golden_manifest, golden_outputs, golden_records

pytestmark = pytest.mark.gpu

K32 = [e for e in golden_manifest() if e["k"] == 32]
UP_TO_PAN = [e["name"] for e in K32][:[e["name"] for e in K32].index("pan_4x20k") + 1]
U64MAX = 2 ** 64 - 1
EINVAL, ESTATE, ERANGE = -1, -4, -5


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


def entry_named(name, k=32):
    return [e for e in golden_manifest() if e["name"] == name and e["k"] == k][0]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


_ROWS, _SAMPLES = {}, {}


def rows_of(api, entry):
    """(records, (words, hash rows, '$' row)) of a golden: its files, or a build that gives the golden's hashes"""
    key = (entry["name"], entry["k"])
    if key not in _ROWS:
        recs = golden_records(entry)
        out = golden_outputs(entry)
        if out is None:
            d = api.DeBWT(k=entry["k"])
            d.load_records(recs)
            d.build()
            out = d.fetch()
            d.close()
            sha = entry["sha256"]
            assert _sha(out[0]) == sha["bwt"] and _sha(out[1]) == sha["hash"]
            assert _sha(np.array([out[2]], dtype=np.uint64)) == sha["dollar"]
        _ROWS[key] = (recs, out)
    return _ROWS[key]


def samples_of(api, entry, s):
    key = (entry["name"], s)
    if key not in _SAMPLES:
        recs, rows = rows_of(api, entry)
        d = api.DeBWT(k=32)
        d.load_records(recs)
        fm = d.fm_index(sa_sample=s, rows=rows)
        _SAMPLES[key] = fm.samples()
        fm.close()
        d.close()
    return _SAMPLES[key]


def opened(api, entry, s, samples=None):
    recs, rows = rows_of(api, entry)
    sa = samples_of(api, entry, s) if samples is None else samples
    return api.FMIndex.open(rows[0], entry["n"], rows[1], rows[2], sa, sa_sample=s)


def strings(recs):
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [lut[np.asarray(r, dtype=np.uint8)].tobytes() for r in recs]


def raw_extract(fm, jobs, capacity=None):
    """(rc, out_offsets, bytes) of one debwt_fm_extract call with jobs (record, reserved, offset, length)"""
    from debwt_amd import _lib
    L = _lib.lib()
    ja = (_lib.DebwtFmExtractJob * max(len(jobs), 1))()
    for k, (rec, res, off, length) in enumerate(jobs):
        ja[k].record, ja[k].reserved, ja[k].offset, ja[k].length = rec, res, off, length
    offs = np.full(len(jobs) + 1, 12345, dtype=np.uint64)
    cap = 1 << 16 if capacity is None else capacity
    buf = ctypes.create_string_buffer(max(cap, 1))
    rc = L.debwt_fm_extract(fm._h, ja, len(jobs), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), buf, cap)
    return rc, offs, buf.raw


@pytest.mark.parametrize("name", UP_TO_PAN)
def test_whole_records(api, name):
    entry = entry_named(name)
    want = strings(rows_of(api, entry)[0])
    for s in (1, 4, 32, 1024):
        fm = opened(api, entry, s)
        got = fm.extract([(r,) for r in range(len(want))])
        st = fm.extract_stats()
        fm.close()
        assert got == want, (name, s)
        assert st["jobs"] == len(want) and st["bases"] == sum(len(w) for w in want) and st["batches"] == 1
        assert 0 < st["bases"] <= st["steps"] <= st["wave_steps"] and st["line_reads"] >= st["steps"]
        assert st["segments"] >= len(want) and st["anchor_bytes"] > 0 and st["ms_kernel"] > 0 and st["ms_wall"] > 0
        if s == 1:
            assert st["segments"] == st["steps"] == st["bases"]       # every position an anchor: segments of one step


def test_t1_at_1024_has_one_segment_over_all_records(api):
    entry = entry_named("t1_three_records")
    sa = samples_of(api, entry, 1024)
    assert len(sa) == 2 and entry["records"] == 3


def test_twenty_thousand_jobs_in_one_call(api):
    entry = entry_named("reads_20000")
    want = strings(rows_of(api, entry)[0])
    assert len(want) == 20000
    fm = opened(api, entry, 32)
    got = fm.extract([(r,) for r in range(len(want))])
    st = fm.extract_stats()
    fm.close()
    assert got == want
    assert st["jobs"] == 20000 and st["batches"] == 1 and st["segments"] > 20000


def substring_jobs(want, sa, starts, seed):
    """2,000 random jobs and the fixed ones, as (record, offset, length); and what each must give"""
    rng = np.random.default_rng(seed)
    jobs = []
    for _ in range(2000):
        r = int(rng.integers(0, len(want)))
        off = int(rng.integers(0, len(want[r]) + 1))
        jobs.append((r, off, int(rng.integers(0, 400))))
    last = len(want) - 1
    jobs += [(0, 7, 0), (1 % len(want), len(want[1 % len(want)]), 10), (0, len(want[0]) - 5, 100), (last, 3, U64MAX),
             (0, 0, 1), (last, len(want[last]) - 1, 1)]
    # a job that begins exactly at a sampled position and one that ends exactly at one
    found = 0
    for p in sorted(int(x) for x in sa):
        r = int(np.searchsorted(starts, p, side="right")) - 1
        off = p - int(starts[r])
        if 1 <= off < len(want[r]):                                      # neither a record's first base nor a separator
            beg = max(0, off - 37)
            jobs += [(r, off, 33), (r, beg, off - beg)]
            found += 1
            if found == 2:
                break
    assert found >= 1
    jobs += [(last, 11, 70)] * 3
    exp = [want[r][off:off + min(length, len(want[r]))] for r, off, length in jobs]
    return jobs, exp


@pytest.mark.parametrize("name", ["t1_three_records", "lowercase_3x2500"])
@pytest.mark.parametrize("s", [4, 1024])
def test_substrings_and_batching(api, monkeypatch, name, s):
    entry = entry_named(name)
    want = strings(rows_of(api, entry)[0])
    fm = opened(api, entry, s)
    jobs, exp = substring_jobs(want, samples_of(api, entry, s), fm.record_starts(), seed=s + len(name))
    got = fm.extract(jobs)
    st = fm.extract_stats()
    assert got == exp
    assert st["jobs"] == len(jobs) and st["bases"] == sum(len(e) for e in exp) and st["batches"] == 1
    # the same jobs cut into batches of 4096 output bytes
    monkeypatch.setenv("DEBWT_FM_EXTRACT_BYTES", "4096")
    got2 = fm.extract(jobs)
    st2 = fm.extract_stats()
    fm.close()
    assert got2 == exp
    assert st2["batches"] > 1 and st2["bases"] == st["bases"] and st2["steps"] >= st["steps"]


def test_long_job_is_split_over_many_segments(api):
    entry = entry_named("single_record")
    want = strings(rows_of(api, entry)[0])
    fm = opened(api, entry, 4)
    got = fm.extract([(0,)])
    st = fm.extract_stats()
    fm.close()
    assert got == want and st["jobs"] == 1
    assert st["segments"] > 1 and st["segments"] >= len(want[0]) // 64


def test_protocol(api):
    entry = entry_named("t1_three_records")
    want = strings(rows_of(api, entry)[0])
    fm = opened(api, entry, 4)
    nrec = len(want)
    before = fm.info()["device_bytes"]
    jobs = [(0, 0, 5, 40), (2, 0, 0, U64MAX), (1, 0, 3, 9)]
    total = 40 + len(want[2]) + 9
    rc, offs, _ = raw_extract(fm, jobs, capacity=total - 1)             # one short: offsets complete, nothing built
    assert rc == ERANGE and offs.tolist() == [0, 40, 40 + len(want[2]), total]
    assert fm.info()["device_bytes"] == before
    rc, offs, raw = raw_extract(fm, jobs, capacity=total)
    assert rc == 0 and offs.tolist() == [0, 40, 40 + len(want[2]), total]
    assert raw[:total] == want[0][5:45] + want[2] + want[1][3:12]
    st = fm.extract_stats()
    after = fm.info()["device_bytes"]
    assert st["anchor_bytes"] > 0 and after - before == st["anchor_bytes"] and st["ms_anchors"] > 0
    assert st["anchor_bytes"] >= 8 * len(samples_of(api, entry, 4))
    rc, _, _ = raw_extract(fm, jobs, capacity=total)
    assert rc == 0 and fm.info()["device_bytes"] == after and fm.extract_stats()["ms_anchors"] == 0
    for bad in ((nrec, 0, 0, 1), (0, 0, len(want[0]) + 1, 1), (1, 1, 0, 1)):
        rc, _, _ = raw_extract(fm, [(0, 0, 0, 3), bad])
        assert rc == EINVAL, bad
        assert fm._L.debwt_fm_last_error(fm._h)
    rc, offs, _ = raw_extract(fm, [(0, 0, len(want[0]), 5)])              # offset == |S| is legal and empty
    assert rc == 0 and offs.tolist() == [0, 0]
    rc, offs, _ = raw_extract(fm, [])
    assert rc == 0 and int(offs[0]) == 0
    assert fm.extract([]) == []
    with pytest.raises(api.DebwtError):
        fm.text()                                                       # no text attached
    fm.close()


def sampled_reads(want, count, seed):
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(count):
        rec = want[int(rng.integers(0, len(want)))]
        L = int(rng.integers(40, 120))
        p = int(rng.integers(0, len(rec) - L))
        s = bytearray(rec[p:p + L])
        for _ in range(int(rng.integers(0, 3))):
            s[int(rng.integers(1, L - 1))] = b"ACGT"[int(rng.integers(0, 4))]
        s = bytes(s)
        reads.append(s.translate(comp)[::-1] if i % 2 else s)
    return reads


@pytest.mark.parametrize("name", ["t1_three_records", "shared_ends_duplicates", "pan_4x20k"])
def test_restore(api, name):
    entry = entry_named(name)
    recs, rows = rows_of(api, entry)
    want = strings(recs)
    n = entry["n"]
    words, n2, sep = api.pack_records(recs)
    assert n2 == n
    body = (n + 63) >> 5
    reads = sampled_reads(want, 200, seed=5)
    d = api.DeBWT(k=32)
    d.load_records(recs)
    ref = d.fm_index(sa_sample=32, rows=rows)
    ref.attach_text(d)
    d.close()
    ref_map = ref.map(reads)
    assert ref_map.mapped.sum() >= 100
    ref.close()
    for s in (1, 32, 1024):
        fm = opened(api, entry, s)
        before = fm.info()["device_bytes"]
        fm.restore_text()
        st = fm.extract_stats()
        assert st["jobs"] == 0 and st["bases"] == n and st["steps"] == n - 1 and st["segments"] >= 1
        assert st["steps"] <= st["wave_steps"] and st["ms_kernel"] > 0
        assert fm.info()["device_bytes"] >= before + n // 4 + st["anchor_bytes"]
        w, sp = fm.text()
        assert len(w) == body + 2 and np.array_equal(w[:body], words[:body]) and not w[body:].any()
        assert np.array_equal(sp, sep)
        held = fm.info()["device_bytes"]
        fm.restore_text()                                                # a text is attached: nothing to do
        w2, sp2 = fm.text()
        assert np.array_equal(w2, w) and np.array_equal(sp2, sp) and fm.info()["device_bytes"] == held
        got = fm.map(reads)
        fm.close()
        assert np.array_equal(got.hits, ref_map.hits) and np.array_equal(got.offsets, ref_map.offsets)
        assert np.array_equal(got.cigars, ref_map.cigars)


def test_refusals(api):
    """corrupted samples: error returns only (every walk is bounded by a difference of checked positions)"""
    entry = entry_named("t1_three_records")
    want = strings(rows_of(api, entry)[0])
    n = entry["n"]
    good = samples_of(api, entry, 4)
    i = len(good) // 2
    swapped = good.copy()
    swapped[[i, i + 1]] = swapped[[i + 1, i]]
    dup = good.copy()
    dup[i + 1] = dup[i]
    cases = [("swapped", swapped, False), ("duplicated", dup, True)]
    for what, sa, extract_refuses in cases:
        assert not np.array_equal(sa, good)
        fm = opened(api, entry, 4, samples=sa)
        with pytest.raises(api.DebwtError) as e:
            fm.restore_text()
        assert e.value.code == EINVAL and fm._L.debwt_fm_last_error(fm._h), what
        with pytest.raises(api.DebwtError) as e:
            fm.extend([want[0][:50]], [(0, 0, 0, 0)])
        assert e.value.code == ESTATE, what
        if extract_refuses:
            with pytest.raises(api.DebwtError) as e:
                fm.extract([(0,)])
            assert e.value.code == EINVAL and fm._L.debwt_fm_last_error(fm._h), what
        fm.close()
    # a sample set to n is no text position: debwt_fm_open itself refuses such samples, so neither restore nor extract
    # ever sees them
    beyond = good.copy()
    beyond[i] = n
    with pytest.raises(api.DebwtError) as e:
        opened(api, entry, 4, samples=beyond)
    assert e.value.code == EINVAL


def test_round_trip_through_another_k(api):
    e32, e20 = entry_named("chrom_1M_5", 32), entry_named("chrom_1M_5", 20)
    fm = opened(api, e32, 32)
    fm.restore_text()
    words, sep = fm.text()
    fm.close()
    d = api.DeBWT(k=20)
    d.load_packed(words, e32["n"], sep)
    d.build()
    w, h, dr = d.fetch()
    d.close()
    sha = e20["sha256"]
    assert _sha(w) == sha["bwt"] and _sha(h) == sha["hash"] and _sha(np.array([dr], dtype=np.uint64)) == sha["dollar"]
