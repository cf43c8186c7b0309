"""Graph cleaning on one GPU (debwt_fm_graph_clean) on reads that had errors, written to a profile.

    python scripts/gpu_fm_clean_bench.py --out profiles/r22_fm_clean.txt

The workload is that of scripts/gpu_fm_kmer_bench.py --part overlaps: a random genome of reads x length / coverage bases,
`reads` reads of `length` bases at uniform positions, forward strand, every base substituted with probability --error; the
reads are corrected at --correct-k (debwt_fm_correct, both strands), the index is rebuilt from the corrected reads at s = 32,
and the string graph over both strands is taken at --min-overlap.  Then the graph is cleaned (max_tip, max_bubble,
max_rounds as given).  Reported: unitigs and N50 before and after, the cleaning's counters, ms_clean (its kernels, by
events) next to ms_reduce of the graph call, and the library-call time of the graph call alone and of graph + clean.
Every time is the median of --reps calls after one untimed call, with the smallest and largest beside it."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_fm_graph_bench import n50, unitig_lengths  # noqa: E402


def spread(v):
    return [round(float(np.median(v)), 2), round(float(min(v)), 2), round(float(max(v)), 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--correct-k", type=int, default=21)
    ap.add_argument("--min-overlap", type=int, default=40)
    ap.add_argument("--max-tip", type=int, default=4)
    ap.add_argument("--max-bubble", type=int, default=16)
    ap.add_argument("--max-rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_clean.txt"))
    args = ap.parse_args()
    from debwt_amd import _lib, api
    L = _lib.lib()
    rng = np.random.default_rng(1)
    n, m = args.reads, args.length
    G = int(n * m / args.coverage)
    genome = rng.integers(0, 4, G).astype(np.uint8)          # the same draws as gpu_fm_kmer_bench.py
    starts = rng.integers(0, G - m + 1, n)
    clean = genome[(starts[:, None] + np.arange(m)[None, :])]
    rng2 = np.random.default_rng(2)
    flip = rng2.random(clean.shape, dtype=np.float32) < args.error
    noisy = np.where(flip, (clean + rng2.integers(1, 4, clean.shape, dtype=np.uint8)) % 4, clean).astype(np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(m)

    def index_of(letters):
        buf = letters.tobytes()
        d = api.DeBWT(k=32)
        d.load_ascii([buf[i * m:(i + 1) * m] for i in range(n)])
        d.build()
        fm = d.fm_index(sa_sample=32)
        d.close()
        return fm, buf

    fm, buf = index_of(acgt[noisy])
    out = ctypes.create_string_buffer(len(buf))
    info = np.zeros(n, dtype=api._CORRECT_DTYPE)
    o = _lib.DebwtFmCorrectOpts(k=args.correct_k, min_count=3, max_rounds=4, flags=1)
    rc = L.debwt_fm_correct(fm._h, buf, api._p64(offs), n, ctypes.byref(o), out, info.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmCorrectInfo)))
    assert rc == 0, fm._L.debwt_fm_last_error(fm._h)
    fixed = np.frombuffer(out.raw, dtype=np.uint8).reshape(n, m)
    fm.close()
    row = {"reads": n, "length": m, "coverage": args.coverage, "genome": G, "error": args.error, "correct_k": args.correct_k,
           "min_overlap": args.min_overlap, "max_tip": args.max_tip, "max_bubble": args.max_bubble, "max_rounds": args.max_rounds,
           "reps": args.reps, "substituted_bases": int(flip.sum()), "wrong_bases_after": int((fixed != acgt[clean]).sum())}
    fm, _ = index_of(fixed)
    reclen = np.full(2 * n, m, dtype=np.int64)

    def shape(g):
        lens, circ = unitig_lengths(g, reclen)
        return {"kept_nodes": int((g.state == 0).sum()), "edges": int(g.offsets[-1]), "unitigs": len(lens), "circular": int(circ.sum()),
                "unitig_bases": int(lens.sum()), "unitig_n50": n50(lens), "unitig_longest": int(lens.max()) if len(lens) else 0,
                "unitigs_of_one_read": int((np.diff(g.unitigs()[0].astype(np.int64)) == 1).sum())}

    kw = dict(max_tip=args.max_tip, max_bubble=args.max_bubble, max_rounds=args.max_rounds)
    g = fm.string_graph_both(min_overlap=args.min_overlap)
    g.clean(**kw)
    lib_graph, lib_clean, ms_reduce, ms_clean, wall_graph, wall_both = [], [], [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        g = fm.string_graph_both(min_overlap=args.min_overlap)
        t1 = time.perf_counter()
        c = g.clean(**kw)
        t2 = time.perf_counter()
        gs, cs = fm.graph_both_stats(), fm.clean_stats()
        lib_graph.append(gs["ms_wall"]); lib_clean.append(cs["ms_wall"])
        ms_reduce.append(gs["ms_reduce"]); ms_clean.append(cs["ms_clean"])
        wall_graph.append((t1 - t0) * 1e3); wall_both.append((t2 - t0) * 1e3)
    row["graph"] = {"ms_library": spread(lib_graph), "ms_reduce": spread(ms_reduce), "python_wall_ms": spread(wall_graph),
                    "ms_kernel": round(sum(gs[k] for k in ("ms_walk", "ms_build", "ms_tail", "ms_merge", "ms_reduce")), 2),
                    "edges_E": gs["edges"], "reducible": gs["reducible"]}
    row["clean"] = {"ms_library": spread(lib_clean), "ms_clean": spread(ms_clean), "python_wall_graph_and_clean_ms": spread(wall_both),
                    "graph_plus_clean_ms_library": spread([a + b for a, b in zip(lib_graph, lib_clean)]),
                    **{k: cs[k] for k in ("nodes", "edges", "rounds", "tips", "tip_nodes", "bubbles", "bubble_nodes", "steps", "launches")}}
    row["before"], row["after"] = shape(g), shape(c)
    row["clipped_nodes"], row["popped_nodes"] = int((c.state == api.NODE_CLIPPED).sum()), int((c.state == api.NODE_POPPED).sum())
    row["ms_clean_over_ms_reduce"] = round(row["clean"]["ms_clean"][0] / max(row["graph"]["ms_reduce"][0], 1e-9), 2)
    fm.close()
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
