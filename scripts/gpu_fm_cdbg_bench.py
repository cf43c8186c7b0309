"""The compacted de Bruijn graph on one GPU (debwt_fm_cdbg), written to a profile.

    python scripts/gpu_fm_cdbg_bench.py --out profiles/r28_fm_cdbg.txt

The two workloads of scripts/gpu_fm_records_bench.py (same functions, same seeds), each in a child process of its own under
--step-timeout seconds (the first failure ends the script): `reads` at every k of --read-ks, `pan` at every k of --pan-ks.
Per workload and k:

part "esa"    debwt_fm_esa_build with max_lcp = k + 1, sa and da: what `deBWT-query dbg` pays before the call (ms_wall, one
              build, and its device bytes).
part "cdbg"   --reps sizing calls and --reps calls that write the graph, each after one untimed: ms per phase (nodes, links,
              rank, write) and ms_wall of the library call, scratch_bytes, nodes, unitigs, circular, edges, longest_nodes,
              jump_rounds, the busy share of the ranking rounds (jump_steps / jump_wave_steps), N50 of the unitig strings.
part "route"  the way without the feature, in the same process: debwt_fm_kmer_list (forward) of k and of k + 1, degrees and
              links by numpy searches over the two code lists, then a Python walk along the links from every first node in
              code order under --route-budget seconds.  The row names how many unitigs it reached; nodes, kmer_count and
              string of each are compared with the library's.
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

from gpu_fm_esa_bench import read_set, spread  # noqa: E402
from gpu_fm_records_bench import pan_genome  # noqa: E402

PHASES = ("ms_nodes", "ms_links", "ms_rank", "ms_write", "ms_wall")
COUNTS = ("nodes", "edge_strings", "unitigs", "circular", "links", "edges", "longest_nodes", "seq_bytes", "jump_rounds",
          "jump_steps", "jump_wave_steps", "rank_lines", "scratch_bytes")


def emit(args, row):
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as out:
        out.write(json.dumps(row) + "\n")


def n50(lengths):
    if not len(lengths):
        return 0
    s = np.sort(lengths)[::-1]
    run = np.cumsum(s)
    return int(s[np.searchsorted(run, (int(run[-1]) + 1) // 2)])


def route(args, fm, k, G):
    """kmer lists of k and k + 1, numpy degrees, a Python walk under a budget; compared with G, the library's answer"""
    t0 = time.perf_counter()
    ck, mk = fm.kmer_list(k, strands="forward")
    ce, _ = fm.kmer_list(k + 1, strands="forward")
    lists = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    N = len(ck)
    mask = np.uint64((1 << (2 * k)) - 1)
    u = np.searchsorted(ck, ce >> np.uint64(2))
    v = np.searchsorted(ck, ce & mask)
    outdeg, indeg = np.bincount(u, minlength=N), np.bincount(v, minlength=N)
    is_link = (outdeg[u] == 1) & (indeg[v] == 1) & (u != v)
    nxt = np.full(N, -1, dtype=np.int64)
    nxt[u[is_link]] = v[is_link]
    has_prev = np.zeros(N, dtype=bool)
    has_prev[v[is_link]] = True
    heads = np.nonzero(~has_prev)[0]
    prep = (time.perf_counter() - t0) * 1e3
    plain = np.nonzero((G.unitigs["flags"] & 1) == 0)[0]          # the walk meets the unitigs that have a first node, in order
    assert len(plain) == len(heads)
    seq, lut = G.seq, np.frombuffer(b"ACGT", dtype=np.uint8)
    t0, done, equal = time.perf_counter(), 0, True
    nx, mult, code = nxt, mk, ck
    while done < len(heads) and time.perf_counter() - t0 < args.route_budget:
        for h in heads[done:done + 2000].tolist():
            nodes, w = [h], nx[h]
            while w >= 0:
                nodes.append(w)
                w = nx[w]
            rec = G.unitigs[plain[done]]
            idx = np.asarray(nodes)
            first = int(code[h])
            s = bytes(lut[[(first >> (2 * (k - 1 - j))) & 3 for j in range(k)]]) + lut[(code[idx[1:]] & np.uint64(3)).astype(np.int64)].tobytes()
            off = int(rec["seq_offset"])
            equal &= (len(nodes) == rec["nodes"] and int(mult[idx].sum()) == rec["kmer_count"]
                      and seq[off:off + len(s)].tobytes() == s)
            done += 1
    loop = (time.perf_counter() - t0) * 1e3
    assert equal
    return {"part": "route", "k": k,
            "what": "debwt_fm_kmer_list (forward) of k and k + 1, degrees and links by numpy searches, a Python walk along the "
                    "links from every first node under a time budget; one run",
            "kmer_lists_ms": round(lists, 1), "degrees_ms": round(prep, 1), "walk_ms": round(loop, 1), "unitigs_done": done,
            "unitigs_with_first_node": len(heads), "walk_ms_extrapolated": round(loop * len(heads) / max(done, 1), 1),
            "equal_to_library": True}


def run(which, args):
    from debwt_amd import _lib, api
    recs, head = read_set(args) if which == "reads" else pan_genome(args)
    d = api.DeBWT(k=32)
    t0 = time.perf_counter()
    d.load_ascii(recs)
    del recs
    d.build()
    fm = d.fm_index(sa_sample=32)
    d.close()
    n, nrec = fm.info()["n"], fm.info()["nrec"]
    head = {"workload": which, **head, "n": n, "nrec": nrec, "index_s": round(time.perf_counter() - t0, 2)}
    for k in (args.read_ks if which == "reads" else args.pan_ks):
        fm.esa(max_lcp=k + 1, sa=True, da=True)                         # the text is restored by the first
        e = fm.esa(max_lcp=k + 1, sa=True, da=True)
        es = fm.esa_stats()
        emit(args, {**head, "part": "esa", "k": k, "max_lcp": k + 1, "esa_build_ms": round(es["ms_wall"], 1),
                    "kept_bytes": es["kept_bytes"], "build_bytes": es["build_bytes"]})

        def sizing():
            sz = _lib.DebwtFmCdbgSizes()
            rc = fm._L.debwt_fm_cdbg(fm._h, k, 0, None, 0, None, 0, None, 0, ctypes.byref(sz))
            assert rc in (0, -5), rc
            return fm.cdbg_stats()

        sizing()
        rows = [sizing() for _ in range(args.reps)]
        G = e.cdbg(k)
        full = []
        for _ in range(args.reps):
            G = e.cdbg(k)
            full.append(fm.cdbg_stats())
        st = full[-1]
        lens = G.unitigs["nodes"].astype(np.int64) + k - 1
        emit(args, {"workload": which, "part": "cdbg", "k": k, "reps": args.reps,
                    "sizing": {p: spread([r[p] for r in rows]) for p in PHASES},
                    "writing": {p: spread([r[p] for r in full]) for p in PHASES},
                    "rank_busy": round(st["jump_steps"] / max(st["jump_wave_steps"], 1), 3),
                    "N50": n50(lens), **{c: st[c] for c in COUNTS}})
        if k + 1 <= 32:
            emit(args, {"workload": which, **route(args, fm, k, G)})
        del G
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
    ap.add_argument("--read-ks", type=int, nargs="+", default=[21, 31])
    ap.add_argument("--pan-ks", type=int, nargs="+", default=[31])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", nargs="+", default=["reads", "pan"])
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--route-budget", type=float, default=20.0, help="seconds of the host walk over the unitigs")
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_cdbg.txt"))
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
               "--reps", str(args.reps), "--route-budget", str(args.route_budget),
               "--read-ks", *[str(c) for c in args.read_ks], "--pan-ks", *[str(c) for c in args.pan_ks]]
        rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        if rc:
            sys.exit(f"{which}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
