"""Distinct records per LCP interval on one GPU (debwt_fm_records_build and what stands on it), written to a profile.

    python scripts/gpu_fm_records_bench.py --out profiles/r27_fm_records.txt

Two workloads, each in a child process of its own under --step-timeout seconds (the first failure ends the script):
`reads`, the 10^6 reads of 100 b at 20x of scripts/gpu_fm_esa_bench.py (same function, same seeds), and `pan`, --copies
copies of one random genome of --genome bases, every base of a copy substituted with probability --divergence.  The
arrays are built once (lcp + sa + da), then:

part "build"    debwt_fm_esa_build beside it (ms_wall of the one build), then per fanout of --fanouts
                (DEBWT_FM_REPEAT_FANOUT; the first stays in force for the other parts) --reps calls of
                debwt_fm_records_build after one untimed: ms per phase (keys and sort, tree, pairs, scan) and ms_wall, pairs, sort passes, rmq_steps,
                the busy share of the pairs kernel (rmq_steps / wave_steps), reads per pair, bytes.
part "repeats"  sizing calls (no list) at --min-len, kind "maximal": debwt_fm_repeats, then debwt_fm_repeats_records with
                the filter that filters nothing, with min_records = --min-records (at most the number of records), with
                unique, and with both (multi-MUMs when that is the number of records): ms_search, ms_wall, reported.
part "counts"   the list of every interval of at least --min-len bases (kind "intervals") is fetched once, then
                debwt_fm_record_counts over all of them: ms_wall of --reps calls (upload of the ranges, gather, download).
part "route"    the way without the feature, in the same process: debwt_fm_esa_fetch of da and lcp to the host, prev[] by
                a stable argsort of da, then per interval np.count_nonzero(prev[lo:hi] < lo), the distinct records of its
                rows.  A Python loop over the intervals in list order under --route-budget seconds: the row names how
                many intervals it got through, and its counts are compared with the library's.
Every list is [median, smallest, largest]."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from gpu_fm_esa_bench import read_set, spread  # noqa: E402


def emit(args, row):
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as out:
        out.write(json.dumps(row) + "\n")


def pan_genome(args):
    rng = np.random.default_rng(4)
    base = rng.integers(0, 4, args.genome, dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for c in range(args.copies):
        g = base.copy()
        if c:
            hit = rng.random(args.genome, dtype=np.float32) < args.divergence
            g[hit] = (g[hit] + rng.integers(1, 4, int(hit.sum()), dtype=np.uint8)) % 4
        out.append(lut[g].tobytes())
    return out, {"genome": args.genome, "copies": args.copies, "divergence": args.divergence}


def run(which, args):
    from debwt_amd import api
    recs, head = read_set(args) if which == "reads" else pan_genome(args)
    d = api.DeBWT(k=32)
    t0 = time.perf_counter()
    d.load_ascii(recs)
    del recs
    d.build()
    fm = d.fm_index(sa_sample=32)
    d.close()
    n, nrec = fm.info()["n"], fm.info()["nrec"]
    e = fm.esa(sa=True, da=True)
    es = fm.esa_stats()
    head = {"workload": which, **head, "n": n, "nrec": nrec, "index_and_arrays_s": round(time.perf_counter() - t0, 2),
            "esa_build_ms": round(es["ms_wall"], 1), "lcp_max": e.summary()["max"]}

    want = None
    for fanout in reversed(args.fanouts):                               # the first of --fanouts last: it stays in force below
        os.environ["DEBWT_FM_REPEAT_FANOUT"] = str(fanout)
        e.records_build()
        rows = []
        for _ in range(args.reps):
            e.records_build()
            rows.append(fm.records_stats())
        st = rows[-1]
        tail = e.dup_prefix(n - 1, n)
        want = tail if want is None else want
        assert st["fanout"] == fanout and np.array_equal(tail, want) and int(tail[0]) == st["pairs"]
        emit(args, {**head, "part": "build", "reps": args.reps,
                    **{k: spread([r[k] for r in rows]) for k in ("ms_sort", "ms_tree", "ms_pairs", "ms_scan", "ms_wall")},
                    "pairs_busy": round(st["rmq_steps"] / max(st["wave_steps"], 1), 3),
                    "reads_per_pair": round(st["rmq_steps"] / max(st["pairs"], 1), 2),
                    **{k: st[k] for k in ("pairs", "records_present", "sort_passes", "levels", "fanout", "rmq_steps", "wave_steps",
                                          "build_bytes", "kept_bytes")}})

    q = min(args.min_records, nrec) if args.min_records else nrec

    # sizing calls at min_len: through the raw protocol, so that no list is written
    import ctypes
    from debwt_amd import _lib

    def call(flt):
        opts = _lib.DebwtFmRepeatOpts(args.min_len, 0, 2, 0)
        cnt = ctypes.c_uint64(0)
        if flt is None:
            rc = fm._L.debwt_fm_repeats(fm._h, ctypes.byref(opts), None, 0, ctypes.byref(cnt))
        else:
            f = _lib.DebwtFmRecordFilter(*flt, 0)
            rc = fm._L.debwt_fm_repeats_records(fm._h, ctypes.byref(opts), ctypes.byref(f), None, None, 0, ctypes.byref(cnt))
        assert rc in (0, -5), rc
        return fm.repeat_stats()

    for name, flt in (("debwt_fm_repeats", None), ("filter {1, 0, 0}", (1, 0, 0)), (f"min_records {q}", (q, 0, 0)),
                      ("unique", (1, 0, 1)), (f"unique, min_records {q}", (q, 0, 1))):
        call(flt)
        rows = [call(flt) for _ in range(args.reps)]
        st = rows[-1]
        emit(args, {"workload": which, "part": "repeats", "call": name, "min_len": args.min_len, "kind": "maximal", "reps": args.reps,
                    **{k: spread([r[k] for r in rows]) for k in ("ms_tree", "ms_search", "ms_wall")},
                    "intervals": st["intervals"], "maximal": st["maximal"], "reported": st["reported"]})

    every, lib = e.repeats_by_record(min_len=args.min_len, kind="intervals")
    rg = np.ascontiguousarray(np.stack([every["row_lo"], every["row_lo"] + every["count"]], axis=1).astype(np.uint64))
    ms = []
    for _ in range(args.reps + 1):
        t = time.perf_counter()
        got = e.record_counts(rg)
        ms.append((time.perf_counter() - t) * 1e3)
    assert np.array_equal(got, lib.astype(np.uint64))
    emit(args, {"workload": which, "part": "counts", "min_len": args.min_len, "intervals": len(rg), "reps": args.reps,
                "ms_wall": spread(ms[1:]), "ranges_MB": round(rg.nbytes / 1e6, 1),
                "below_count": int(np.count_nonzero(lib < every["count"]))})

    # the route without the feature
    t0 = time.perf_counter()
    da, lcp = e.da(), e.lcp()
    fetch = (time.perf_counter() - t0) * 1e3
    del lcp                                                             # fetched as the route must; the list stands for its walk
    t0 = time.perf_counter()
    order = np.argsort(da, kind="stable")
    prev = np.full(n, -1, dtype=np.int64)
    same = da[order[1:]] == da[order[:-1]]
    prev[order[1:][same]] = order[:-1][same]
    prep = (time.perf_counter() - t0) * 1e3
    t0, done = time.perf_counter(), 0
    host = np.zeros(len(rg), dtype=np.uint64)
    while done < len(rg) and time.perf_counter() - t0 < args.route_budget:
        for lo, hi in rg[done:done + 10000].tolist():
            host[done] = np.count_nonzero(prev[lo:hi] < lo)
            done += 1
    loop = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(host[:done], got[:done])
    emit(args, {"workload": which, "part": "route",
                "what": "debwt_fm_esa_fetch of da and lcp, prev[] by a stable argsort of da, then np.count_nonzero(prev[lo:hi] < lo) "
                        "per interval in a Python loop under a time budget; one run",
                "fetch_da_lcp_ms": round(fetch, 1), "prev_ms": round(prep, 1), "loop_ms": round(loop, 1), "intervals_done": done,
                "intervals": len(rg), "loop_ms_extrapolated": round(loop * len(rg) / max(done, 1), 1), "equal_to_library": True})
    fm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--genome", type=int, default=1 << 24)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--divergence", type=float, default=0.01)
    ap.add_argument("--min-len", type=int, default=20)
    ap.add_argument("--min-records", type=int, default=8, help="at most the records of the index; 0: every record")
    ap.add_argument("--fanouts", type=int, nargs="+", default=[64, 16], help="of the build; the first is in force for the rest")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", nargs="+", default=["reads", "pan"])
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--route-budget", type=float, default=20.0, help="seconds of the host loop over the intervals")
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_records.txt"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        run(args.child, args)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for which in args.workloads:                                  # a fresh process per workload; a failure ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--out", args.out, "--reads", str(args.reads),
               "--length", str(args.length), "--coverage", str(args.coverage), "--error", str(args.error),
               "--genome", str(args.genome), "--copies", str(args.copies), "--divergence", str(args.divergence),
               "--min-len", str(args.min_len), "--min-records", str(args.min_records), "--reps", str(args.reps),
               "--route-budget", str(args.route_budget), "--fanouts", *[str(c) for c in args.fanouts]]
        rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        if rc:
            sys.exit(f"{which}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
