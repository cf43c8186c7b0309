"""The string graph on one GPU (debwt_fm_string_graph): kernel time per phase, the library call, and the counts of kept
records, edges, irreducible edges and unitigs with their N50, beside what a user could do before on the same reads and
index -- debwt_fm_overlaps with DEBWT_FM_OVERLAP_LONGEST -- measured again in the same run, written to a profile.

    python scripts/gpu_fm_graph_bench.py --out profiles/r20_fm_graph.txt

The workload is that of scripts/gpu_fm_overlap_bench.py: a random genome of reads x length / coverage bases, `reads`
reads of `length` bases drawn from it at uniform positions (forward strand only), their BWT and index at s = 32, the
reads against their own index with min_overlap (default 40).  Every figure is the median of --reps calls after one
untimed call of the same shape, with the smallest and largest beside it.  ms_walk (state search, unpacking, walk,
compaction, expansion), ms_build (packing, longest per pair, compaction into E) and ms_reduce (reduction, compaction of
the kept edges) are sums of launches by events; ms_library is the host time of one debwt_fm_string_graph call with a
capacity that fits; wall_ms is FMIndex.string_graph, which calls the library a second time when its first buffer was too
small.  The unitig lengths are computed from the record lengths and overlaps, without extracting the sequences."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def n50(lengths):
    v = np.sort(np.asarray(lengths, dtype=np.int64))[::-1]
    return int(v[np.searchsorted(np.cumsum(v), (int(v.sum()) + 1) // 2)]) if len(v) else 0


def unitig_lengths(g, reclen):
    uoff, mem, circ = g.unitigs()
    deg = (g.offsets[1:] - g.offsets[:-1]).astype(np.int64)
    first = np.zeros(len(reclen), dtype=np.int64)              # the length of a record's first out-edge, 0 without one
    has = deg > 0
    first[has] = g.edges["length"][g.offsets[:-1][has].astype(np.int64)]
    give = reclen[mem].astype(np.int64) - first[mem]           # every member but the last: |S| - L_next
    last = uoff[1:].astype(np.int64) - 1
    open_end = last[circ == 0]
    give[open_end] = reclen[mem[open_end]]                     # the last member of a linear unitig is whole
    return np.add.reduceat(give, uoff[:-1].astype(np.int64)) if len(circ) else np.zeros(0, np.int64), circ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--min-overlap", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_graph.txt"))
    args = ap.parse_args()
    from debwt_amd import api
    rng = np.random.default_rng(1)
    G = int(args.reads * args.length / args.coverage)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, G)]
    starts = rng.integers(0, G - args.length + 1, args.reads)
    flat = genome[(starts[:, None] + np.arange(args.length)[None, :]).ravel()].tobytes()
    rs = [flat[i * args.length:(i + 1) * args.length] for i in range(args.reads)]
    d = api.DeBWT(k=32)
    d.load_ascii(rs)
    d.build()
    fm = d.fm_index(sa_sample=32)
    d.close()
    res = {"reads": args.reads, "length": args.length, "coverage": args.coverage, "genome": G, "n": fm.n,
           "min_overlap": args.min_overlap, "reps": args.reps}

    def spread(v):
        return [round(float(np.median(v)), 2), round(float(min(v)), 2), round(float(max(v)), 2)]

    # the yardstick: the longest overlaps of every read, as before this section existed
    fm.overlaps(rs, min_overlap=args.min_overlap, longest=True)
    wall, kern, lib = [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        r = fm.overlaps(rs, min_overlap=args.min_overlap, longest=True)
        wall.append((time.perf_counter() - t0) * 1e3)
        st = fm.overlaps_stats()
        kern.append(st["ms_kernel"])
        lib.append(st["ms_wall"])
    res["overlaps_longest"] = {"hits": int(r.offsets[-1]), "wall_ms": spread(wall), "ms_kernel": spread(kern),
                               "ms_library": spread(lib)}
    print(json.dumps(res["overlaps_longest"]), flush=True)
    del r
    reclen = np.full(args.reads, args.length, dtype=np.int64)
    for reduce in (True, False):
        fm.string_graph(min_overlap=args.min_overlap, reduce=reduce)
        wall, lib, phase = [], [], {"ms_walk": [], "ms_build": [], "ms_reduce": []}
        for _ in range(args.reps):
            t0 = time.perf_counter()
            g = fm.string_graph(min_overlap=args.min_overlap, reduce=reduce)
            wall.append((time.perf_counter() - t0) * 1e3)
            st = fm.graph_stats()
            lib.append(st["ms_wall"])
            for k in phase:
                phase[k].append(st[k])
        row = {"reduce": reduce, "wall_ms": spread(wall), "ms_library": spread(lib)}
        row.update({k: spread(v) for k, v in phase.items()})
        row["ms_kernel"] = spread([a + b + c for a, b, c in zip(*phase.values())])
        row.update({k: st[k] for k in ("kept", "duplicates", "contained", "hits", "edges", "reducible", "lookups", "launches")})
        row["returned_edges"] = int(g.offsets[-1])
        row["scratch_GB"] = round(st["scratch_bytes"] / 1e9, 2)
        row["edge_GB"] = round(st["edge_bytes"] / 1e9, 3)
        row["max_out_degree"] = int((g.offsets[1:] - g.offsets[:-1]).max())
        if reduce:
            row["reduce_over_walk"] = round(float(np.median(phase["ms_reduce"])) / float(np.median(phase["ms_walk"])), 3)
            row["lookups_per_edge"] = round(st["lookups"] / max(st["edges"], 1), 2)
            t0 = time.perf_counter()
            lens, circ = unitig_lengths(g, reclen)
            row["unitigs_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row.update({"unitigs": len(lens), "circular": int(circ.sum()), "unitig_bases": int(lens.sum()), "unitig_n50": n50(lens),
                        "unitig_longest": int(lens.max()) if len(lens) else 0})
        row["library_over_overlaps_longest"] = round(float(np.median(lib)) / res["overlaps_longest"]["ms_library"][0], 2)
        row["kernel_over_overlaps_longest"] = round(row["ms_kernel"][0] / res["overlaps_longest"]["ms_kernel"][0], 2)
        res.setdefault("runs", []).append(row)
        print(json.dumps(row), flush=True)
        del g
    fm.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as out:
        out.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
