"""Maximal repeats from the kept LCP array on one GPU (debwt_fm_repeats), written to a profile.

    python scripts/gpu_fm_repeats_bench.py --out profiles/r26_fm_repeats.txt

The two workloads of scripts/gpu_fm_esa_bench.py (same functions, same seeds), each in a child process of its own under
--step-timeout seconds (the first failure ends the script): `reads`, 10^6 reads of 100 b at 20x, and `genome`, one record
of 2^28 random bases with 200 copied stretches of 20,000 bases.  The arrays are built once (lcp + sa), then per fanout
of --fanouts and per min_len of --min-lens, kind "maximal":

part "count"   the sizing call (no list: tree and search alone), --reps calls after one untimed: ms_tree, ms_search and
               ms_wall, the busy share of the search (search_steps / wave_steps), reads per row searched, the counts.
part "list"    at the first fanout only: the call that writes the list into a host array of `reported` records: ms_tree,
               ms_search, ms_write, ms_wall, scratch.
part "route"   the way without the feature, in the same process: debwt_fm_esa_fetch of lcp and sa to the host, then the
               interval ends of every row with lcp >= min_len on the host.  The one-pass stack of tests/repeat_ref.py is
               a Python loop over n rows; what runs here is a NUMPY RESTATEMENT of it, named as such: nearest smaller values
               by pointer jumping (p[r] <- p[p[r]] while lcp[p[r]] > lcp[r], all rows of a round at once), representatives
               and interval ends only -- no left counts, no flags, no list in order, so it is a lower bound of that route.
               Its number of intervals is compared with the library's.
Every list is [median, smallest, largest]."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from gpu_fm_esa_bench import genome, read_set, spread  # noqa: E402


def emit(args, row):
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as out:
        out.write(json.dumps(row) + "\n")


def host_intervals(lcp, min_len):
    """numpy restatement of the stack walk: the number of intervals with l >= min_len, and their ends"""
    n = len(lcp)
    v = np.concatenate([lcp.astype(np.int64), [-1]])                    # a sentinel below everything behind the last row
    rows = np.nonzero(lcp >= min_len)[0]
    l = v[rows]
    p = np.arange(-1, n, dtype=np.int64)                                # p[r] = r - 1: nothing between p[r] and r
    p[0] = 0
    act, rounds = rows, 0
    while len(act):                                                     # left: the nearest value <= l
        act = act[v[p[act]] > v[act]]
        p[act] = p[p[act]]
        rounds += 1
    q = np.arange(1, n + 2, dtype=np.int64)                             # q[r] = r + 1; q[n] = n + 1 is never read
    q[n] = n
    act = rows
    while len(act):                                                     # right: the nearest value < l
        act = act[v[q[act]] >= v[act]]
        q[act] = q[q[act]]
        rounds += 1
    rep = v[p[rows]] < l
    return int(rep.sum()), p[rows][rep], q[rows][rep] - 1, rounds


def run(which, args):
    from debwt_amd import _lib, api
    recs, head = read_set(args) if which == "reads" else genome(args)
    d = api.DeBWT(k=32)
    t0 = time.perf_counter()
    d.load_ascii(recs)
    del recs
    d.build()
    fm = d.fm_index(sa_sample=32)
    d.close()
    n = fm.info()["n"]
    e = fm.esa(sa=True)
    es = fm.esa_stats()
    head = {"workload": which, **head, "n": n, "nrec": fm.info()["nrec"], "index_and_arrays_s": round(time.perf_counter() - t0, 2),
            "esa_build_ms": round(es["ms_wall"], 1), "lcp_max": e.summary()["max"]}

    def call(min_len, out=None):
        opts = _lib.DebwtFmRepeatOpts(min_len, 0, 2, 0)
        cnt = ctypes.c_uint64(0)
        rc = fm._L.debwt_fm_repeats(fm._h, ctypes.byref(opts), None if out is None else out.ctypes.data_as(ctypes.c_void_p),
                                    0 if out is None else len(out), ctypes.byref(cnt))
        assert rc in ((0, -5) if out is None else (0,)), rc
        return fm.repeat_stats()

    keys = ("rows", "searched", "representatives", "intervals", "maximal", "supermaximal", "reported", "longest_len", "levels",
            "tree_bytes", "scratch_bytes")
    want = {}
    for fanout in args.fanouts:
        os.environ["DEBWT_FM_REPEAT_FANOUT"] = str(fanout)
        for min_len in args.min_lens:
            call(min_len)
            rows = [call(min_len) for _ in range(args.reps)]
            st = rows[-1]
            want.setdefault(min_len, st["intervals"])
            assert st["intervals"] == want[min_len] and st["fanout"] == fanout
            emit(args, {**head, "part": "count", "fanout": fanout, "min_len": min_len, "reps": args.reps,
                        **{k: spread([r[k] for r in rows]) for k in ("ms_tree", "ms_search", "ms_wall")},
                        "search_busy": round(st["search_steps"] / max(st["wave_steps"], 1), 3),
                        "reads_per_row_searched": round(st["search_steps"] / max(st["searched"], 1), 2),
                        "rank_lines": st["rank_lines"], **{k: st[k] for k in keys}})
    os.environ["DEBWT_FM_REPEAT_FANOUT"] = str(args.fanouts[0])
    for min_len in args.min_lens:
        out = np.zeros(max(call(min_len)["reported"], 1), dtype=api.REPEAT_DTYPE)
        rows = [call(min_len, out) for _ in range(args.reps)]
        st = rows[-1]
        assert st["reported"] == len(out) or st["reported"] == 0
        emit(args, {"workload": which, "part": "list", "fanout": args.fanouts[0], "min_len": min_len, "reps": args.reps,
                    **{k: spread([r[k] for r in rows]) for k in ("ms_tree", "ms_search", "ms_write", "ms_wall")},
                    "reported": st["reported"], "list_MB": round(out.nbytes / 1e6, 1), "scratch_MB": round(st["scratch_bytes"] / 1e6, 1)})
        del out
    # the route without the feature
    t0 = time.perf_counter()
    lcp, sa = e.lcp(), e.sa()
    fetch = (time.perf_counter() - t0) * 1e3
    del sa
    spent = 0.0
    for min_len in args.min_lens:
        if spent > args.route_budget:                                   # the walk before took that long: this one is not run
            emit(args, {"workload": which, "part": "route", "min_len": min_len, "skipped": f"{spent:.0f} s spent on the host already"})
            continue
        t0 = time.perf_counter()
        cnt, lo, hi, rounds = host_intervals(lcp, min_len)
        ms = (time.perf_counter() - t0) * 1e3
        spent += ms / 1e3
        assert cnt == want[min_len], (cnt, want[min_len])
        emit(args, {"workload": which, "part": "route", "min_len": min_len,
                    "what": "debwt_fm_esa_fetch of lcp and sa, then a numpy restatement of the stack walk (pointer jumping; interval "
                            "ends only, no left counts, no order), one run",
                    "fetch_lcp_sa_ms": round(fetch, 1), "host_intervals_ms": round(ms, 1), "rounds": rounds, "intervals": cnt,
                    "equal_to_library": True})
    fm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--genome", type=int, default=1 << 28)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--repeat-length", type=int, default=20000)
    ap.add_argument("--fanouts", type=int, nargs="+", default=[64, 32, 16])
    ap.add_argument("--min-lens", type=int, nargs="+", default=[20, 1])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", nargs="+", default=["reads", "genome"])
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--route-budget", type=float, default=120.0, help="seconds of host walks after which no further one starts")
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_repeats.txt"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        run(args.child, args)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for which in args.workloads:                                  # a fresh process per workload; a failure ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--out", args.out, "--reads", str(args.reads),
               "--length", str(args.length), "--coverage", str(args.coverage), "--error", str(args.error),
               "--genome", str(args.genome), "--repeats", str(args.repeats), "--repeat-length", str(args.repeat_length),
               "--reps", str(args.reps), "--route-budget", str(args.route_budget), "--fanouts", *[str(c) for c in args.fanouts], "--min-lens", *[str(c) for c in args.min_lens]]
        rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        if rc:
            sys.exit(f"{which}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
