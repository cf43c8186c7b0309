"""The string graph over both strands on one GPU (debwt_fm_string_graph_both) beside the route there was before it: the
strand-0 graph (debwt_fm_string_graph) of an index built from the doubled collection (S_0, rc S_0, S_1, ...), measured in
the same run and written to a profile.

    python scripts/gpu_fm_bigraph_bench.py --out profiles/r21_fm_graph_both.txt

The workload is that of scripts/gpu_fm_graph_bench.py -- a random genome of reads x length / coverage bases, `reads` reads
of `length` bases at uniform positions, index at s = 32, min_overlap 40 -- with every read reverse-complemented with
probability 1/2.  (A) is string_graph_both on the index of the reads, (B) string_graph on the index of the doubled reads.
Every figure is the median of --reps calls after one untimed call of the same shape, with the smallest and largest beside
it; the ms_* phases are sums of launches by events, ms_library the host time of the library call.  Both must return the
same three arrays (a SHA-1 of state, offsets and edges is compared) and so the same oriented unitigs.  The build columns
are the wall time of the BWT build and of the index (rank structure and samples), and device_bytes that of the index."""
import argparse
import hashlib
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


def digest(g):
    h = hashlib.sha1()
    for a in (g.state, g.offsets, g.edges):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def index_of(api, rows):
    """(index, BWT build ms, index build ms) of the reads in the rows of a 2-D array of ASCII bases"""
    flat, length = rows.tobytes(), rows.shape[1]
    rs = [flat[i * length:(i + 1) * length] for i in range(rows.shape[0])]
    d = api.DeBWT(k=32)
    t0 = time.perf_counter()
    d.load_ascii(rs)
    d.build()
    t1 = time.perf_counter()
    fm = d.fm_index(sa_sample=32)
    t2 = time.perf_counter()
    d.close()
    return fm, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--min-overlap", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_graph_both.txt"))
    args = ap.parse_args()
    from debwt_amd import api
    rng = np.random.default_rng(1)
    G = int(args.reads * args.length / args.coverage)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, G)]
    starts = rng.integers(0, G - args.length + 1, args.reads)
    fwd = genome[starts[:, None] + np.arange(args.length)[None, :]]
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    flip = rng.random(args.reads) < 0.5
    reads = np.where(flip[:, None], comp[fwd[:, ::-1]], fwd)
    both = np.stack([reads, comp[reads[:, ::-1]]], axis=1).reshape(2 * args.reads, args.length)
    res = {"reads": args.reads, "length": args.length, "coverage": args.coverage, "genome": G, "min_overlap": args.min_overlap,
           "reps": args.reps, "flipped": int(flip.sum())}
    reclen = np.full(2 * args.reads, args.length, dtype=np.int64)
    phases = {"A": ("ms_walk", "ms_build", "ms_tail", "ms_merge", "ms_reduce"), "B": ("ms_walk", "ms_build", "ms_reduce")}
    for name, rows in (("A", reads), ("B", both)):
        fm, ms_bwt, ms_index = index_of(api, rows)
        call = fm.string_graph_both if name == "A" else fm.string_graph
        stats = fm.graph_both_stats if name == "A" else fm.graph_stats
        call(min_overlap=args.min_overlap)
        wall, lib, phase = [], [], {k: [] for k in phases[name]}
        for _ in range(args.reps):
            t0 = time.perf_counter()
            g = call(min_overlap=args.min_overlap)
            wall.append((time.perf_counter() - t0) * 1e3)
            st = stats()
            lib.append(st["ms_wall"])
            for k in phase:
                phase[k].append(st[k])
        row = {"route": name, "n": fm.n, "device_bytes": fm.info()["device_bytes"], "build_bwt_ms": round(ms_bwt, 1),
               "build_index_ms": round(ms_index, 1), "wall_ms": spread(wall), "ms_library": spread(lib)}
        row.update({k: spread(v) for k, v in phase.items()})
        row["ms_kernel"] = spread([sum(t) for t in zip(*phase.values())])
        row.update({k: st[k] for k in ("kept", "duplicates", "contained", "hits", "edges", "reducible", "lookups", "launches")})
        row["scratch_GB"] = round(st["scratch_bytes"] / 1e9, 2)
        row["edge_GB"] = round(st["edge_bytes"] / 1e9, 3)
        row["returned_edges"] = int(g.offsets[-1])
        row["sha1"] = digest(g)
        if name == "A":
            row.update({k: st[k] for k in ("selfrc", "seeds", "seed_rows", "tail_hits", "edges_kind")})
            row["seed_rows_per_seed"] = round(st["seed_rows"] / max(st["seeds"], 1), 2)
            med = {k: float(np.median(v)) for k, v in phase.items()}
            row["tail_over_walk"] = round(med["ms_tail"] / med["ms_walk"], 3)
            row["merge_over_walk"] = round(med["ms_merge"] / med["ms_walk"], 3)
        # the oriented unitigs of the arrays (the same call folds B's mirror pairs)
        folded = api.BiGraphResult(fm, g.state, g.offsets, g.edges, True)
        lens, circ = unitig_lengths(folded, reclen)
        row.update({"unitigs": len(lens), "circular": int(circ.sum()), "unitig_bases": int(lens.sum()), "unitig_n50": n50(lens),
                    "unitig_longest": int(lens.max()) if len(lens) else 0})
        res.setdefault("runs", []).append(row)
        print(json.dumps(row), flush=True)
        del g, folded
        fm.close()
    a, b = res["runs"]
    res["same_arrays"] = a["sha1"] == b["sha1"]
    res["same_unitigs"] = (a["unitigs"], a["unitig_n50"]) == (b["unitigs"], b["unitig_n50"])
    res["A_over_B"] = {"ms_kernel": round(a["ms_kernel"][0] / b["ms_kernel"][0], 2), "ms_library": round(a["ms_library"][0] / b["ms_library"][0], 2),
                       "device_bytes": round(a["device_bytes"] / b["device_bytes"], 2),
                       "build_ms": round((a["build_bwt_ms"] + a["build_index_ms"]) / (b["build_bwt_ms"] + b["build_index_ms"]), 2)}
    print(json.dumps({k: res[k] for k in ("same_arrays", "same_unitigs", "A_over_B")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as out:
        out.write(json.dumps(res) + "\n")
    if not (res["same_arrays"] and res["same_unitigs"]):
        sys.exit("the two routes disagree")


if __name__ == "__main__":
    main()
