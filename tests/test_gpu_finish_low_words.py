"""Bucket finish in its low-word form (rlw_rounds<true>): where the buckets are cut at bit 32 or below
(pshift <= 32) a wave tile arrives ordered by its high words, so the merge-split rounds compare whole keys but fetch,
select and exchange low words only.  Sorted arrays and everything built from them stay bit-identical.

Every case runs in a fresh child process under a time limit.  DEBWT_PREFIX_DIGITS forces the number of prefix digits, so
that a few thousand keys reach the path that otherwise needs more than 2^30: one digit of a 40-bit key cuts at bit 32, of
a 34-bit key at bit 26 (the high word then holds two bits of the digit).  DEBWT_FINISH_LOW=0 takes the whole-key form as
the comparison.  Expected values: np.sort and the committed golden outputs.

Sizes: a wave tile holds RLW_CAP = 1024 keys, 16 per lane, on a raster of RLW_H = 896; a bucket that starts a tile fits
up to 1024 keys and is unfit from 1025.  The passes in front of the finish are stable, so the keys of a bucket reach the
finish in the order of the input: the descending and reversed cases are laid out for that.  (The tests cannot see the array
between the passes and the finish; a case asks for np.sort's order whatever the rounds found.)

Which form a sort took is read from debwt_radix_low_finishes(); every stand-alone case sorts its keys in both forms."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_manifest, golden_outputs

pytestmark = pytest.mark.gpu

CAP, H, KPT = 1024, 896, 16
KEY_BITS = (40, 34)

CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
job = json.loads(sys.argv[2])
import os
from debwt_amd import api
lows = lambda: int(api._lib.lib().debwt_radix_low_finishes())
res = {}
if job["what"] == "sort":
    import torch
    import test_gpu_finish_low_words as T
    d = api.DeBWT(k=32)
    def sort(keys, kb):
        dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
        tmp = torch.empty_like(dk)
        before = lows()
        d.radix_sort_device(dk.data_ptr(), tmp.data_ptr(), len(keys), kb)
        return dk.cpu().numpy().view(np.uint64), lows() - before
    for kb in job["key_bits"]:
        keys = T.make_keys(job["case"], kb)
        want = np.sort(keys)
        out, took = sort(keys, kb)                                  # the switches are read at every sort
        os.environ["DEBWT_FINISH_LOW"] = "0"
        out0, took0 = sort(keys, kb)
        del os.environ["DEBWT_FINISH_LOW"]
        res[str(kb)] = {"low": bool(np.array_equal(out, want)), "whole": bool(np.array_equal(out0, want)),
                        "low_finishes": took, "low_finishes_whole": took0}
    d.close()
else:
    if job["what"] == "golden":
        from conftest import golden_manifest, golden_records
        recs = golden_records(next(e for e in golden_manifest() if e["name"] == job["name"] and e["k"] == 32))
    else:
        from debwt_amd import synth
        recs = synth.pan_genome(300_000, 3)
    d = api.DeBWT(k=32)
    d.load_records(recs)
    d.set_range_cap(4096)
    d.build()
    api.write_outputs(job["out"], *d.fetch())
    res["low_finishes"] = lows()
    if job["what"] == "pan":
        res["inverse_bwt_ok"] = bool(d.verify_device()["inverse_bwt_ok"])
    d.close()
print("RESULT " + json.dumps(res))
"""


def _child(job, digits, low=None):
    env = dict(os.environ, DEBWT_PREFIX_DIGITS=str(digits))
    env.pop("DEBWT_FINISH_LOW", None)
    if low is not None:
        env["DEBWT_FINISH_LOW"] = low
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(job)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])


def _buckets(parts, shift):
    """keys of the buckets `parts` = [(prefix digit, low parts in the order they are to arrive), ...]"""
    return np.concatenate([(np.uint64(p) << np.uint64(shift)) | np.asarray(low, dtype=np.uint64) for p, low in parts])


def make_keys(case, key_bits):
    """keys of a case: the top 8 of `key_bits` bits are the bucket, the rest the low part; called in the child process"""
    rng = np.random.default_rng(sum(map(ord, case)) + key_bits)
    shift = key_bits - 8
    top = (1 << shift) - 1
    rnd = lambda m: rng.integers(0, 1 << shift, size=m, dtype=np.uint64)                # noqa: E731
    if case.startswith("bucket_") and case[7:].isdigit():           # one bucket of N keys at the start of a tile
        return _buckets([(7, rnd(int(case[7:]))), (11, rnd(5))], shift)
    if case == "bucket_1025_unfit":                                 # one key more than a tile: the stretch is unfit
        return _buckets([(3, rnd(20)), (7, rnd(CAP + 1)), (11, rnd(30)), (12, rnd(900)), (13, rnd(40))], shift)
    if case == "lanes_16_aligned":                                  # every bucket is one lane's 16 keys
        return _buckets([(1 + i, rnd(KPT)) for i in range(64)], shift)
    if case == "lanes_16_shifted":                                  # ... one key later: every bucket lies across a lane boundary
        return _buckets([(0, rnd(1))] + [(1 + i, rnd(KPT)) for i in range(55)] + [(60, rnd(KPT - 1))], shift)
    if case == "bucket_48_descending":                              # slots 10 .. 57: four lanes, the keys want the far end
        return _buckets([(2, rnd(10)), (7, np.sort(rnd(48))[::-1]), (11, rnd(10))], shift)
    if case == "tile_1024_reversed":                                # 64 rounds would be needed: RL_MAX_ROUNDS, then the network
        return _buckets([(7, np.sort(rnd(CAP))[::-1]), (11, rnd(5))], shift)
    if case == "all_equal":
        return np.full(1000, (7 << shift) | 0x2345_6789 & top, dtype=np.uint64)
    if case == "low_extremes":                                      # low parts 0 and all ones, the last bucket next to the padding
        ext = lambda m: rng.permutation(np.concatenate([rnd(m), np.zeros(9, np.uint64), np.full(9, top, np.uint64)]))   # noqa: E731
        return _buckets([(7, ext(300)), (254, ext(100)), (255, ext(200))], shift)
    if case == "high_words_differ_in_bit_32":                       # with 40-bit keys: the digits 6 / 7 and 4 / 5
        return _buckets([(4, rnd(50)), (5, rnd(50)), (6, rnd(100)), (7, rnd(100))], shift)
    if case == "short_last_tile":                                   # 56 lanes of one bucket each, then a tile of 7 keys
        return _buckets([(1 + i, rnd(KPT)) for i in range(56)] + [(200, rnd(7))], shift)
    raise KeyError(case)


SORT_CASES = ["bucket_1", "bucket_15", "bucket_16", "bucket_17", "bucket_1023", "bucket_1024", "bucket_1025_unfit",
              "lanes_16_aligned", "lanes_16_shifted", "bucket_48_descending", "tile_1024_reversed", "all_equal",
              "low_extremes", "high_words_differ_in_bit_32", "short_last_tile"]


@pytest.mark.parametrize("case", SORT_CASES)
def test_stand_alone_sort(case):
    """one prefix digit: 40-bit keys are cut at bit 32, 34-bit keys at bit 26; both forms of the finish give np.sort's
    order, and the counter of the library says which form each sort took"""
    r = _child({"what": "sort", "case": case, "key_bits": KEY_BITS}, digits=1)
    for kb in KEY_BITS:
        assert r[str(kb)]["low_finishes"] == 1 and r[str(kb)]["low_finishes_whole"] == 0, kb
        assert r[str(kb)]["low"], kb
        assert r[str(kb)]["whole"], kb


def test_prefix_digits_switch():
    """DEBWT_PREFIX_DIGITS=4 on 100 keys of 64 bits (the rule gives them one digit): still np.sort's order"""
    r = _child({"what": "sort", "case": "bucket_95", "key_bits": (64,)}, digits=4)
    assert r["64"]["low_finishes"] == 1 and r["64"]["low_finishes_whole"] == 0      # four digits of 64 bits: cut at bit 32
    assert r["64"]["low"] and r["64"]["whole"]
    r1 = _child({"what": "sort", "case": "bucket_95", "key_bits": (64,)}, digits=1)  # one digit: cut at bit 56, whole keys
    assert r1["64"]["low_finishes"] == 0 and r1["64"]["low"]


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


@pytest.mark.parametrize("name", ["t1_three_records", "homopolymers_tandem"])
def test_golden_build_with_four_prefix_digits(name, tmp_path):
    """k = 32 with four forced digits: the counting finish cuts at bit 32; the smallest entry and one full of repeats"""
    entry = next(e for e in golden_manifest() if e["name"] == name and e["k"] == 32)
    files = golden_outputs(entry)
    assert files is not None
    low, whole = str(tmp_path / "low"), str(tmp_path / "whole")
    assert _child({"what": "golden", "name": name, "out": low}, digits=4)["low_finishes"] > 0
    assert _child({"what": "golden", "name": name, "out": whole}, digits=4, low="0")["low_finishes"] == 0
    for out in (low, whole):
        assert np.fromfile(out, dtype=np.uint64).tobytes() == files[0].tobytes()
        assert np.fromfile(out + ".#", dtype=np.uint64).tobytes() == files[1].tobytes()
        assert int(np.fromfile(out + ".$", dtype=np.uint64)[0]) == files[2]
        for ext, key in (("", "bwt"), (".#", "hash"), (".$", "dollar")):
            assert _sha(out + ext) == entry["sha256"][key], ext
    for ext in ("", ".#", ".$"):
        assert open(low + ext, "rb").read() == open(whole + ext, "rb").read(), ext


def test_pan_genome_build_both_ways(tmp_path):
    low, whole = str(tmp_path / "low"), str(tmp_path / "whole")
    r1 = _child({"what": "pan", "out": low}, digits=4)
    r0 = _child({"what": "pan", "out": whole}, digits=4, low="0")
    assert r1["low_finishes"] > 0 and r0["low_finishes"] == 0
    assert r1["inverse_bwt_ok"] and r0["inverse_bwt_ok"]
    for ext in ("", ".#", ".$"):
        assert open(low + ext, "rb").read() == open(whole + ext, "rb").read(), ext
