"""Every k from 12 to 32 through every form of the build, on the two texts of tests/k_ladder.py (structure at every
length from 10 to 34; tests/test_k_ladder_ref.py shows on the CPU that a neighbouring K gives other intermediates).

The expected values come from the oracle and from the definition of the keys, once per text at module scope: BWT words,
'#' rows and '$' row once (they do not depend on k), stats, red array and SP symbols per k.  Groups:

  (a) stage by stage, both texts: sorted keys, distinct keys, red array, SP symbols, k-mer counts, stats, row symbols, BWT
  (b) the forms of the key sort inside a build of `mid`: DEBWT_PREFIX_DIGITS x DEBWT_BUCKET_PASS x DEBWT_FINISH_LOW,
      DEBWT_HIST_EVERY_PASS, sort_algo 1, tune 256 / 32768 / 131072 / 8388608 -- in one key range and under range caps of
      4096 and 20000; which form ran is read from the library's counters and compared with radix_split's rule (radix_sort.h),
      restated below: never from a first run
  (c) the sort primitive at the builder's key widths against np.sort
  (d) SP stage and prefilter switches on `mid`
  (e) the special-region module on the device (DEBWT_SPECIAL_DEVICE_MIN=0)
  (f) unfit and oversize stretches of the key sort (the `runs` and `copies` texts of tests/test_gpu_parity.py, and `runs4`)
  (g) three shards on one GPU, both key modes
  (h) the two switches a process reads once: DEBWT_SPARSE_LOCKSTEP and DEBWT_OVER_PLAIN, a fresh child process each

The comparisons are the check_* functions below: tests/test_k_sweep_selfcheck.py feeds them right and hand-made wrong
values on the CPU and shows that they pass and fail where they should.

sort_unfit_stretches / sort_unfit_network / sort_over_stretches of (f) are path indicators, not results (asserted where
OVER_PATH_KS below says why, printed with every case).  As measured on an MI355X they are the same at every k from 12 to
32, because a bucket of these texts is cut by the first 8 symbols of a node whatever k is:
  runs    unfit 5, network 0 (tune 32768: 4), over 1      at k = 12, 13, ..., 32
  copies  unfit 86, network 0 (tune 32768: 23..25), over 0  at k = 12, 13, ..., 32
  runs4   see unfit_records: two oversize stretches at the least are what the compacted form of that path needs"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import k_ladder as KL
from conftest import ROOT

pytestmark = pytest.mark.gpu

KS = KL.KS
TEXTS = ("small", "mid")
CAPS = (None, 4096, 20000)
SORT_ENV = ("DEBWT_PREFIX_DIGITS", "DEBWT_BUCKET_PASS", "DEBWT_FINISH_LOW", "DEBWT_HIST_EVERY_PASS")
STAT_NAMES = ("red_capacity", "blue_capacity", "blue_bound_num", "sp_len", "special_branch_num")
# (f): k of each class 2k % 8 at which the oversize path must run on `runs` (the classes' first and last k; 32 and 21 as in
# test_unfit_stretches_of_the_key_sort_by_classes).  Why every k reaches it: the text's ~45,000 keys take two prefix digits,
# a bucket is the keys that share their first 8 symbols, and of the 14,000 windows of the long run 0.9^8 = 43 % (~6,000,
# above the 4096 keys of a tile) begin with 8 unsubstituted symbols whatever k is.
OVER_PATH_KS = (12, 13, 14, 15, 21, 29, 30, 31, 32)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from debwt_amd import api as A
    return A


@pytest.fixture(scope="module")
def exp(oracle):
    return {name: KL.expected(name) for name in TEXTS}


# ---- the comparisons (also run on the CPU by tests/test_k_sweep_selfcheck.py) ----------------------------------------

def check_keys(sorted_keys, distinct_keys, want_sorted, tag=None):
    assert np.array_equal(sorted_keys, want_sorted), tag
    assert np.array_equal(distinct_keys, np.unique(want_sorted)), tag


def check_stage_arrays(E, k, red, sp, tag=None):
    assert np.array_equal(red, E.red[k]), tag
    assert np.array_equal(sp, E.sp[k]), tag


def check_stats(E, k, st, names=STAT_NAMES, tag=None):
    for nm in names:
        assert st[nm] == E.stats[k][nm], (nm, st[nm], E.stats[k][nm], tag)


def check_result(E, words, hrows, drow, rows=None, tag=None):
    assert np.array_equal(words, E.words), tag
    assert np.array_equal(hrows, E.hrows) and drow == E.drow, tag
    if rows is not None:
        assert np.array_equal(rows, E.rows), tag


def check_kmer_counts(got, want, tag=None):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), tag


def check_counters(want, got, tag=None):
    """want / got: name -> value; a wanted value is an int (equal) or (">=", int)"""
    for nm, w in want.items():
        if isinstance(w, tuple):
            assert got[nm] >= w[1], (nm, got[nm], w, tag)
        else:
            assert got[nm] == w, (nm, got[nm], w, tag)


def check_hashes(want, got, tag=None):
    assert set(got) == set(want), (sorted(set(want) ^ set(got)), tag)
    for key in want:
        assert got[key] == want[key], (key, tag)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def sha_bwt(words, hrows, drow):
    return sha(words, hrows, np.array([drow], dtype=np.uint64))


# ---- radix_split (radix_sort.h) restated ---------------------------------------------------------------------------------

RS_BUCKET_TARGET = 64


def radix_split(n, key_bits, algo, ranged, env):
    """How radix_sort_u64(n keys, key_bits, algo) divides the key bits: None when every digit goes by LSD passes (algo 1,
    no prefix digit, or key_bits - 8 T < 1), else T, pshift = key_bits - 8 T, whether the lowest prefix digit goes by the
    bucket pass (DEBWT_BUCKET_PASS=1: wherever there is a second prefix digit, and two digits at least unless
    DEBWT_PREFIX_DIGITS says otherwise; 0: never; unset: a key range of four digits) and whether the bucket finish takes
    its low-word form (pshift <= 32 unless DEBWT_FINISH_LOW=0).  ranged: the caller vouches for bounds of the keys."""
    bp = env.get("DEBWT_BUCKET_PASS")
    mode = -1 if bp in (None, "") else int(int(bp) != 0)
    forced = int(env.get("DEBWT_PREFIX_DIGITS") or 0)
    T = 0
    while (n >> (8 * T)) > RS_BUCKET_TARGET and T < 4:
        T += 1
    if mode == 1 and T < 2:
        T = 2
    if 1 <= forced <= 4:
        T = forced
    if algo != 3 or T == 0 or key_bits - 8 * T < 1:
        return None
    pshift = key_bits - 8 * T
    fl = env.get("DEBWT_FINISH_LOW")
    return {"T": T, "pshift": pshift, "bucket": T >= 2 if mode == 1 else (mode != 0 and T == 4 and ranged),
            "low": pshift <= 32 and (fl in (None, "") or int(fl) != 0)}


def range_sizes(name, k, cap):
    """keys per key range of a one-GPU build under debwt_set_range_cap(cap): the cut of tests/shard_cases.py (near-equal
    ranges of whole 12-bit prefix bins), by definition of the keys"""
    import shard_cases as SC
    keys = KL.sorted_keys(name, k)
    if cap is None or len(keys) <= cap:
        return [len(keys)]
    hist = np.bincount((keys >> np.uint64(2 * k - 12)).astype(np.int64), minlength=SC.SHARD_BINS).astype(np.int64)
    b = SC.cut_ranges(hist, 0, SC.SHARD_BINS, cap)
    return [int(hist[b[i]:b[i + 1]].sum()) for i in range(len(b) - 1)]


def expected_sort_counters(name, k, cap, env, algo):
    """What a build must add to the counters.  The key sort of every range is radix_sort_u64(M keys, 2k bits, bounds of the
    range when there are several); the auxiliary sorts of a build (facts of a multi-range classification) have 2k bits too
    and no bounds.  With DEBWT_PREFIX_DIGITS the split does not depend on the number of keys, so every sort of the build
    takes the same form and a form that cannot run leaves its counter alone."""
    sizes = range_sizes(name, k, cap)
    splits = [radix_split(m, 2 * k, algo, len(sizes) > 1, env) for m in sizes]
    nbucket = sum(1 for s in splits if s and s["bucket"])
    nlow = sum(1 for s in splits if s and s["low"])
    want = {"stat_bucket_passes": nbucket}
    uniform = bool(env.get("DEBWT_PREFIX_DIGITS")) or algo != 3
    aux_bucket_possible = env.get("DEBWT_BUCKET_PASS") == "1"          # unset: only a RANGE of four digits; 0: never
    want["bucket_passes"] = (">=", nbucket) if nbucket and aux_bucket_possible else nbucket
    want["low_finishes"] = (">=", nlow) if nlow or not uniform else 0
    if env.get("DEBWT_HIST_EVERY_PASS"):
        want["pair_passes"] = 0
    if uniform:                                                        # no range may differ from the others
        assert nbucket in (0, len(sizes)) and nlow in (0, len(sizes))
    return want


def _counters(api):
    L = api._lib.lib()
    return {"bucket_passes": int(L.debwt_radix_bucket_passes()), "low_finishes": int(L.debwt_radix_low_finishes()),
            "pair_passes": int(L.debwt_radix_pair_passes())}


def _ctx(api, recs, k, tune=0, algo=0, cap=None):
    d = api.DeBWT(k=k, sort_algo=algo, tune=tune)
    if cap:
        d.set_range_cap(cap)
    d.load_records(recs)
    return d


def _set_env(monkeypatch, env, names=SORT_ENV):
    for nm in names:
        monkeypatch.delenv(nm, raising=False)
    for nm, v in env.items():
        monkeypatch.setenv(nm, v)


def _finish(d, api, with_rows=False):
    d.classify()
    d.sp_generate()
    d.blue_sort()
    d.bwt_assemble()
    return d.fetch() + ((d.fetch_array(api.ARR_ROW_SYMBOLS),) if with_rows else ())


# ---- (a) stage by stage ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", TEXTS)
def test_a_stage_by_stage(api, oracle, exp, name, k):
    E = exp[name]
    d = _ctx(api, KL.records(name), k)
    for rep in range(2):
        tag = (name, k, rep)
        d.kmer_sort_rle()
        check_keys(d.fetch_array(api.ARR_SORTED_KEYS), d.fetch_array(api.ARR_DISTINCT_KEYS), KL.sorted_keys(name, k), tag)
        d.classify()
        red = d.fetch_array(api.ARR_RED)
        d.sp_generate()
        check_stage_arrays(E, k, red, d.fetch_array(api.ARR_SP_SYMBOLS), tag)
        d.blue_sort()
        d.bwt_assemble()
        words, hrows, drow = d.fetch()
        check_stats(E, k, d.stats(), tag=tag)
        check_result(E, words, hrows, drow, d.fetch_array(api.ARR_ROW_SYMBOLS), tag)
    check_kmer_counts(d.kmer_count_sorted(), oracle.kmer_count(E.sym, k), (name, k))
    d.close()


# ---- (b) forms of the sort inside a build -----------------------------------------------------------------------------------

GRID = [dict({"DEBWT_PREFIX_DIGITS": str(T), "DEBWT_BUCKET_PASS": str(bp)}, **({"DEBWT_FINISH_LOW": "0"} if fl == 0 else {}))
        for T in (1, 2, 3, 4) for bp in (0, 1) for fl in (None, 0)]
# (environment, sort_algo, tune): the switches are read at every sort, so one context takes the whole grid in turn
FORMS = [(env, 0, 0) for env in GRID] + [({"DEBWT_HIST_EVERY_PASS": "1"}, 0, 0), ({}, 1, 0)] + \
        [({}, 0, tune) for tune in (256, 32768, 131072, 8388608)]


@pytest.mark.parametrize("k", KS)
def test_b_sort_forms_inside_a_build(api, exp, k, monkeypatch):
    E, recs, want_keys = exp["mid"], KL.records("mid"), KL.sorted_keys("mid", k)
    for cap in CAPS:
        ctx = {}
        for env, algo, tune in FORMS:
            tag = (k, cap, env, algo, tune)
            if (algo, tune) not in ctx:
                ctx[algo, tune] = _ctx(api, recs, k, tune=tune, algo=algo, cap=cap)
            d = ctx[algo, tune]
            _set_env(monkeypatch, env)
            want = expected_sort_counters("mid", k, cap, env, algo or 3)
            before = _counters(api)
            if cap is None:
                d.kmer_sort_rle()
                check_keys(d.fetch_array(api.ARR_SORTED_KEYS), d.fetch_array(api.ARR_DISTINCT_KEYS), want_keys, tag)
                words, hrows, drow = _finish(d, api)
            else:
                d.build()
                words, hrows, drow = d.fetch()
            st = d.stats()
            got = {nm: v - before[nm] for nm, v in _counters(api).items()}
            got["stat_bucket_passes"] = st["sort_bucket_passes"]
            check_result(E, words, hrows, drow, tag=tag)
            check_stats(E, k, st, tag=tag)
            check_counters(want, got, tag)
            if tune == 256:
                assert st["sort_unfit_stretches"] == 0, tag       # no counting finish: nothing counts its stretches
        for d in ctx.values():
            d.close()


# ---- (c) the sort primitive at the builder's key widths ------------------------------------------------------------------------

KEY_BITS = tuple(range(24, 65, 2)) + (1, 7, 8, 9, 31, 33, 63)
COUNTS = (4097, 20_001)


def primitive_keys(key_bits, count, shared, bounded):
    """(keys, key_lo, key_hi).  The top digit of a key is its top min(key_bits, 8) bits.  bounded: it takes 3 values (2 where
    it has one bit) and the bounds say so, else any value and no bounds.  shared: all keys share everything above bit 8."""
    rng = np.random.default_rng(1000 * key_bits + count + 2 * shared + bounded)
    tb = min(key_bits, 8)
    shift = key_bits - tb
    nv = min(3, 1 << tb)
    base = 37 if (1 << tb) > 40 else 0
    if bounded:
        top = rng.integers(0, nv, size=count, dtype=np.uint64) + np.uint64(base)
        top[:nv] = np.arange(nv, dtype=np.uint64) + np.uint64(base)
    else:
        top = rng.integers(0, 1 << tb, size=count, dtype=np.uint64)
    low = rng.integers(0, 1 << shift, size=count, dtype=np.uint64) if shift else np.zeros(count, dtype=np.uint64)
    if shared and shift:
        m = np.uint64((1 << min(8, shift)) - 1)
        top[:] = top[0]
        low = (low[0] & ~m) | (low & m)
    keys = (top << np.uint64(shift)) | low
    return keys, (base << shift if bounded else 0), ((base + nv) << shift if bounded else 0)


@pytest.mark.parametrize("key_bits", KEY_BITS)
def test_c_sort_primitive(api, key_bits, monkeypatch):
    import torch
    d = api.DeBWT(k=32)
    for count in COUNTS:
        for shared in (False, True):
            for bounded in (False, True):
                keys, lo, hi = primitive_keys(key_bits, count, shared, bounded)
                assert int(keys.max()) >> key_bits == 0 if key_bits < 64 else True
                want_sorted = np.sort(keys)
                src = torch.from_numpy(keys.view(np.int64))
                tmp = torch.empty(count, dtype=torch.int64, device="cuda")
                for env in GRID:
                    tag = (key_bits, count, shared, bounded, env)
                    _set_env(monkeypatch, env)
                    sp = radix_split(count, key_bits, 3, bounded, env)
                    want = {"bucket_passes": int(bool(sp and sp["bucket"])), "low_finishes": int(bool(sp and sp["low"]))}
                    dk = src.cuda()
                    before = _counters(api)
                    d.radix_sort_device(dk.data_ptr(), tmp.data_ptr(), count, key_bits, key_lo=lo, key_hi=hi)
                    got = {nm: v - before[nm] for nm, v in _counters(api).items()}
                    assert np.array_equal(dk.cpu().numpy().view(np.uint64), want_sorted), tag
                    check_counters(want, got, tag)
    d.close()


# ---- (d) SP stage and prefilter thresholds -------------------------------------------------------------------------------------

SP_TUNES = (2048, 4096, 4096 + 6, 4096 + 16384, 4194304, 4096 + 4194304, 2097152)


@pytest.mark.parametrize("k", KS)
def test_d_sp_stage_and_prefilter_switches(api, exp, k):
    """plain bitmap prefilter, minimizer prefilter (no minimizers for K < 16: the bits must change nothing), its filter cut to
    1/4, the node table addressed by minimizer, the SP stage in slices of 2^17 positions, '#' rows by masks"""
    E, recs = exp["mid"], KL.records("mid")
    for tune in SP_TUNES:
        tag = (k, tune)
        d = _ctx(api, recs, k, tune=tune)
        d.kmer_sort_rle()
        d.classify()
        d.sp_generate()
        sp = d.fetch_array(api.ARR_SP_SYMBOLS)
        assert np.array_equal(sp, E.sp[k]), tag
        d.blue_sort()
        d.bwt_assemble()
        words, hrows, drow = d.fetch()
        check_stats(E, k, d.stats(), ("sp_len", "blue_capacity", "red_capacity"), tag)
        check_result(E, words, hrows, drow, tag=tag)
        d.close()


# ---- (e) the special-region module on the device ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k,max_rounds", [(k, None) for k in KS] + [(k, r) for k in (12, 17, 25, 32) for r in ("0", "2")])
def test_e_special_region_module_on_the_device(api, exp, k, max_rounds, monkeypatch):
    monkeypatch.setenv("DEBWT_SPECIAL_DEVICE_MIN", "0")
    if max_rounds is not None:
        monkeypatch.setenv("DEBWT_SPECIAL_MAX_ROUNDS", max_rounds)
    for name in TEXTS:
        for cap in (None, 4096):
            tag = (name, k, cap, max_rounds)
            d = _ctx(api, KL.records(name), k, cap=cap)
            d.build()
            words, hrows, drow = d.fetch()
            st = d.stats()
            d.close()
            assert st["special_path"] == 2, tag
            check_stats(exp[name], k, st, ("special_branch_num",), tag)
            check_result(exp[name], words, hrows, drow, tag=tag)


# ---- (f) unfit and oversize stretches -----------------------------------------------------------------------------------------

_unfit = {}


def unfit_records(name):
    """`runs` and `copies` of tests/test_gpu_parity.py.  `runs` has ONE stretch above 4096 keys (its run of 14,000), and the
    compacted form of the oversize path (rs_over_move with a base per stretch: wb + rb <= key_bits - 8) needs two at least,
    so `runs4` has a run of 14,000 of every symbol, 10 % substitutions each: four buckets of ~6,000 keys."""
    from test_gpu_parity import _unfit_case
    if name != "runs4":
        return _unfit_case(name)
    rng = np.random.default_rng(4243)
    parts = []
    for c in range(4):
        run = np.full(14_000, c, dtype=np.uint8)
        hit = rng.random(len(run)) < 0.10
        run[hit] = (run[hit] + rng.integers(1, 4, size=int(hit.sum()))) & 3
        parts += [rng.integers(0, 4, size=3000).astype(np.uint8), run]
    return [np.concatenate(parts), rng.integers(0, 4, size=900).astype(np.uint8)]


def _unfit_text(name, oracle):
    """(records, row symbols of the BWT by the oracle: one build, they do not depend on k)"""
    if name not in _unfit:
        recs = unfit_records(name)
        sym = oracle.sym_from_codes(recs)
        w, h, dr, _ = oracle.build_bwt(sym, 32)
        _unfit[name] = (recs, oracle.unpack_bwt(w, len(sym), h, dr), {})
    return _unfit[name]


@pytest.mark.parametrize("tune", [0, 32768])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["runs", "copies", "runs4"])
def test_f_unfit_and_over_stretches(api, oracle, name, k, tune):
    recs, want_rows, keys_of = _unfit_text(name, oracle)
    if k not in keys_of:
        keys_of[k] = np.sort(KL.node_keys(recs, k))
    d = _ctx(api, recs, k, tune=tune)
    for rep in range(2):
        d.kmer_sort_rle()
        check_keys(d.fetch_array(api.ARR_SORTED_KEYS), d.fetch_array(api.ARR_DISTINCT_KEYS), keys_of[k], (name, k, tune, rep))
        st = d.stats()
        paths = (name, k, tune, "unfit", st["sort_unfit_stretches"], "network", st["sort_unfit_network"], "over", st["sort_over_stretches"])
        print("PATHS", *paths)
        if k in (32, 21):
            assert st["sort_unfit_stretches"] > 0, paths
        if name in ("runs", "runs4") and k in OVER_PATH_KS:
            assert st["sort_over_stretches"] >= (1 if name == "runs" else 2), paths
        rows = _finish(d, api, with_rows=True)[3]
        assert np.array_equal(rows, want_rows), paths
    d.close()


# ---- (g) shards -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_g_three_shards_on_one_gpu(api, exp, k):
    E = exp["mid"]
    m = api.MultiDeBWT([0, 0, 0], k=k)
    try:
        m.load_records(KL.records("mid"))
        for cap in (None,) + ((20000,) if k in (13, 17, 25, 31) else ()):
            if cap:
                for r in range(3):
                    assert api._lib.lib().debwt_set_range_cap(m._shard_ctx(r), cap) == 0
            for mode in ("exchange", "rescan"):
                m.set_key_mode(mode)
                m.build()
                check_result(E, *m.fetch(), tag=(k, cap, mode))
                _, s0 = m.stats()
                check_stats(E, k, s0, ("red_capacity", "sp_len", "special_branch_num"), (k, cap, mode))
        assert m.verify_device()["ok"] == 1, k
    finally:
        m.close()


# ---- (h) the switches a process reads once ------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
job = json.loads(sys.argv[2])
from debwt_amd import api
import k_ladder as KL
import test_k_sweep_gpu as T
if job["text"] == "mid":
    recs = KL.records("mid")
else:
    recs = T.unfit_records(job["text"])
res = {}
for k in job["ks"]:
    for cap in job["caps"]:
        d = api.DeBWT(k=k)                   # (an error of a build call raises: the child stops there)
        if cap:
            d.set_range_cap(cap)
        d.load_records(recs)
        if cap:
            d.build()
        else:
            d.kmer_sort_rle()
            res["keys-%d" % k] = T.sha(d.fetch_array(api.ARR_SORTED_KEYS))
            res["over-%d" % k] = int(d.stats()["sort_over_stretches"])
            d.classify(); d.sp_generate(); d.blue_sort(); d.bwt_assemble()
        res["bwt-%d-%d" % (k, cap)] = T.sha_bwt(*d.fetch())
        d.close()
print("RESULT " + json.dumps(res))
"""


def _child(job, switch):
    env = dict(os.environ)
    env[switch] = "1"
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(job)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])


def expected_hashes(ks, caps, keys_of, bwt_sha):
    want = {}
    for k in ks:
        for cap in caps:
            if not cap:
                want["keys-%d" % k] = sha(keys_of(k))
            want["bwt-%d-%d" % (k, cap)] = bwt_sha
    return want


def test_h_first_pass_of_a_key_range_in_lockstep(exp):
    """DEBWT_SPARSE_LOCKSTEP=1: the first pass of a key range by the kernel whose waves collect a tile together"""
    caps = [0, 4096, 20000]
    got = _child({"text": "mid", "ks": list(KS), "caps": caps}, "DEBWT_SPARSE_LOCKSTEP")
    E = exp["mid"]
    want = expected_hashes(KS, caps, lambda k: KL.sorted_keys("mid", k), sha_bwt(E.words, E.hrows, E.drow))
    check_hashes(want, {key: v for key, v in got.items() if not key.startswith("over-")})


@pytest.mark.parametrize("name,least", [("runs", 1), ("runs4", 2)])
def test_h_oversize_stretches_by_plain_passes(oracle, name, least):
    """DEBWT_OVER_PLAIN=1: the gathered oversize stretches by passes over whole keys instead of compacted ones (the switch
    decides for two stretches and more: `runs4`; `runs`, with one, must not mind it)"""
    recs, _, _ = _unfit_text(name, oracle)
    got = _child({"text": name, "ks": list(KS), "caps": [0]}, "DEBWT_OVER_PLAIN")
    ow, oh, od, _ = oracle.build_bwt(oracle.sym_from_codes(recs), 32)
    want = expected_hashes(KS, [0], lambda k: np.sort(KL.node_keys(recs, k)), sha_bwt(ow, oh, od))
    check_hashes(want, {key: v for key, v in got.items() if not key.startswith("over-")}, name)
    for k in OVER_PATH_KS:
        assert got["over-%d" % k] >= least, (name, k, got["over-%d" % k])
