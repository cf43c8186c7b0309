"""Bucket pass of the key sort: the lowest prefix digit is split bucket by bucket in LDS (rs_bucket_digit_kernel) instead of
by a count and a scatter pass in HBM.  Sorted arrays and everything built from them stay bit-identical.
Every case runs in a fresh child process with DEBWT_BUCKET_PASS=1, which takes the bucket pass in every sort and gives
every sort two prefix digits at least, and asserts that the kernel ran (debwt_radix_bucket_passes).

Sizes: the kernel reads windows of CAP = 8192 keys, a bucket that fills a window is split in two reads of global memory,
and a tile of the raster is H = 4 CAP keys: a bucket fits or not by the window alone, so the fit edge is CAP / CAP + 1
keys (there is no CAP - H); buckets of CAP / 2 and CAP / 2 + 1 keys, the edge of a raster of half a window, stay in.
Up to 2^22 keys a forced sort has two prefix digits, so the buckets are the values of the top byte; above it three, and
the buckets are the values of the top two bytes."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_manifest, golden_outputs, golden_records

pytestmark = pytest.mark.gpu

CAP, H = 4096, 4 * 4096

CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
job = json.loads(sys.argv[2])
from debwt_amd import api
passes = lambda: int(api._lib.lib().debwt_radix_bucket_passes())
res = {}
if job["what"] == "sort":
    import torch
    import test_gpu_bucket_pass as T
    keys, lo, hi = T.make_keys(job["case"])
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    tmp = torch.empty_like(dk)
    d = api.DeBWT(k=32)
    d.radix_sort_device(dk.data_ptr(), tmp.data_ptr(), len(keys), 64, key_lo=lo, key_hi=hi)
    out = dk.cpu().numpy().view(np.uint64)
    d.close()
    res["equal"] = bool(np.array_equal(out, np.sort(keys)))
elif job["what"] == "build":
    from conftest import golden_manifest, golden_records
    entry = next(e for e in golden_manifest() if e["name"] == job["name"] and e["k"] == 32)
    d = api.DeBWT(k=32)
    d.load_records(golden_records(entry))
    d.set_range_cap(4096)
    d.build()
    res["stat"] = int(d.stats()["sort_bucket_passes"])
    api.write_outputs(job["out"], *d.fetch())
    d.close()
else:
    from debwt_amd import synth
    m = api.MultiDeBWT([0, 0], k=32)
    m.load_records(synth.pan_genome(300_000, 3))
    m.set_key_mode(job["mode"])
    m.build()
    api.write_outputs(job["out"], *m.fetch())
    m.close()
res["passes"] = passes()
print("RESULT " + json.dumps(res))
"""


def _child(job, force="1"):
    env = dict(os.environ, DEBWT_BUCKET_PASS=force)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(job)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])


def _from_buckets(sizes, tops, rng, low_bits=56, shift=56):
    """keys of the given bucket sizes: bucket i holds sizes[i] keys with the prefix tops[i] at `shift`, the rest random"""
    pre = np.repeat(np.asarray(tops, dtype=np.uint64), sizes) << np.uint64(shift)
    keys = pre | rng.integers(0, 1 << low_bits, size=len(pre), dtype=np.uint64)
    return keys[rng.permutation(len(keys))]


def make_keys(case):
    """(keys, key_lo, key_hi) of a stand-alone case; called in the child process"""
    rng = np.random.default_rng(sum(map(ord, case)))
    B = 37
    if case in ("uniform_2p18", "uniform_2p18_plus_13"):
        n = (1 << 18) + (13 if case.endswith("13") else 0)
        keys = ((rng.integers(0, 3, size=n, dtype=np.uint64) + np.uint64(B)) << np.uint64(56)) | rng.integers(0, 1 << 56, size=n, dtype=np.uint64)
        return keys, B << 56, (B + 3) << 56
    if case == "long_bucket_empty_neighbours":                  # 2^17 keys: one bucket above the window, nothing beside it
        return _from_buckets([(1 << 17) - 300, 300], [B + 1, B + 5], rng), B << 56, (B + 8) << 56
    if case == "raster_fit_edge":                               # the window's edges, buckets that end on and cross tile starts
        sizes = [CAP // 2, CAP // 2 + 1, CAP, CAP + 1, 1, CAP - 1, CAP // 2 - 1, 2 * CAP, 7, CAP - 8, 1, 1]
        sizes += [2 * H - sum(sizes), H, 3, H + 1, CAP]         # ... a bucket that ends on a tile start, one that is a whole tile
        return _from_buckets(sizes, [B + 2 * i for i in range(len(sizes))], rng), B << 56, (B + 2 * len(sizes)) << 56
    if case == "many_buckets":                                  # 200 buckets of 1 .. 12,000 keys: several per window, some across it
        sizes = rng.integers(1, 12000, size=200)
        sizes[::7] = rng.integers(1, 40, size=len(sizes[::7]))
        return _from_buckets(list(sizes), [B + i for i in range(200)], rng), B << 56, (B + 200) << 56
    if case == "three_digits":                                  # above 2^22 keys: buckets by the top two bytes, ~5,500 keys each
        n = (1 << 22) + 4099
        keys = ((rng.integers(0, 3, size=n, dtype=np.uint64) + np.uint64(B)) << np.uint64(56)) | rng.integers(0, 1 << 56, size=n, dtype=np.uint64)
        return keys, B << 56, (B + 3) << 56
    if case == "all_equal":
        return np.full(1 << 17, (B << 56) | 0x1234_5678_9ABC, dtype=np.uint64), B << 56, (B + 1) << 56
    if case == "one_bucket_one_digit":                          # the top two bytes shared: every lane adds to one counter
        keys = (np.uint64((B << 8 | 0x5C) << 48)) | rng.integers(0, 1 << 48, size=1 << 17, dtype=np.uint64)
        return keys, B << 56, (B + 1) << 56
    if case in ("one_key", "two_keys"):
        keys = np.array([(B << 56) | 99, (B << 56) | 5][:1 if case == "one_key" else 2], dtype=np.uint64)
        return keys, B << 56, (B + 1) << 56
    raise KeyError(case)


@pytest.mark.parametrize("case", ["uniform_2p18", "uniform_2p18_plus_13", "long_bucket_empty_neighbours", "raster_fit_edge",
                                  "many_buckets", "three_digits", "all_equal", "one_bucket_one_digit", "one_key", "two_keys"])
def test_stand_alone_sort(case):
    r = _child({"what": "sort", "case": case})
    assert r["passes"] > 0
    assert r["equal"]


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


@pytest.mark.parametrize("name", ["t1_three_records", "special_branches", "pan_4x20k"])
def test_build_in_key_ranges_of_4096(name, tmp_path):
    entry = next(e for e in golden_manifest() if e["name"] == name and e["k"] == 32)
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    r = _child({"what": "build", "name": name, "out": on})
    assert r["passes"] > 0 and r["stat"] > 0
    r0 = _child({"what": "build", "name": name, "out": off}, force="0")
    assert r0["passes"] == 0 and r0["stat"] == 0
    for ext, key in (("", "bwt"), (".#", "hash"), (".$", "dollar")):
        assert open(on + ext, "rb").read() == open(off + ext, "rb").read(), ext
        assert _sha(on + ext) == entry["sha256"][key], ext
    files = golden_outputs(entry)
    if files is not None:
        assert np.array_equal(np.fromfile(on, dtype=np.uint64), files[0])
        assert np.array_equal(np.fromfile(on + ".#", dtype=np.uint64), files[1])
        assert int(np.fromfile(on + ".$", dtype=np.uint64)[0]) == files[2]


def test_two_shards_in_one_process(oracle, tmp_path):
    from debwt_amd import synth
    ow, oh, od, _ = oracle.build_bwt(oracle.sym_from_codes(synth.pan_genome(300_000, 3)), 32)
    for mode in ("exchange", "rescan"):
        out = str(tmp_path / mode)
        r = _child({"what": "multi", "mode": mode, "out": out})
        assert r["passes"] > 0
        assert np.array_equal(np.fromfile(out, dtype=np.uint64), ow)
        assert np.array_equal(np.fromfile(out + ".#", dtype=np.uint64), oh)
        assert int(np.fromfile(out + ".$", dtype=np.uint64)[0]) == od
