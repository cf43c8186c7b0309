"""Suffix-prefix overlaps on one GPU (debwt_fm_overlaps): kernel and wall time, hits per second and the share of lanes
busy, beside debwt_fm_count on the same reads and index, written to a profile.

    python scripts/gpu_fm_overlap_bench.py --out profiles/r13_fm_overlaps.txt

A random genome of reads x length / coverage bases, `reads` reads of `length` bases drawn from it at uniform positions
(forward strand only), their BWT and index at s = 32; then the reads are queried against their own index with
min_overlap (default 40), forward and on both strands, and with the longest reduction, --reps times each after one
untimed call of the same shape; every figure is the median, with the smallest and largest beside it.  ms_kernel sums the walk,
compaction and expansion launches by events; ms_library is the host time of the last debwt_fm_overlaps call (upload,
launches, download, the sort by record inside equal lengths); wall_ms is FMIndex.overlaps, which calls the library a
second time when its first buffer was too small.  busy = rank steps / wave steps.  The yardstick is debwt_fm_count on the
same reads: the walk is a count walk (which stops earlier: count walks the whole read, the overlap walk stops at the
first empty interval) plus two binary searches over the separator rows per step past min_overlap."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--min-overlap", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_overlaps.txt"))
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
    t0 = time.perf_counter()
    d.build()
    build_s = time.perf_counter() - t0
    fm = d.fm_index(sa_sample=32)
    d.close()
    res = {"reads": args.reads, "length": args.length, "coverage": args.coverage, "genome": G, "n": fm.n,
           "min_overlap": args.min_overlap, "build_s": round(build_s, 3), "runs": []}

    def spread(v):
        return [round(float(np.median(v)), 2), round(float(min(v)), 2), round(float(max(v)), 2)]

    fm.count(rs)
    cs = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        cnt = fm.count(rs)
        cs.append((time.perf_counter() - t0) * 1e3)
    assert int(cnt.min()) >= 1
    count_ms = float(np.median(cs))
    res["count_wall_ms"] = spread(cs)
    res["count_reads_per_s"] = round(args.reads / count_ms * 1e3)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}), flush=True)
    for strands, longest in (("forward", False), ("both", False), ("forward", True)):
        fm.overlaps(rs, min_overlap=args.min_overlap, strands=strands, longest=longest)   # the record table, the scratch
        wall, kern, lib = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = fm.overlaps(rs, min_overlap=args.min_overlap, strands=strands, longest=longest)
            wall.append((time.perf_counter() - t0) * 1e3)
            st = fm.overlaps_stats()
            kern.append(st["ms_kernel"])
            lib.append(st["ms_wall"])
        nh = int(r.offsets[-1])
        mk, ml = float(np.median(kern)), float(np.median(lib))
        row = {"strands": strands, "longest": longest, "reps": args.reps, "wall_ms": spread(wall), "ms_kernel": spread(kern),
               "ms_library": spread(lib), "hits": nh, "runs": st["runs"], "hits_per_read": round(nh / args.reads, 2),
               "hits_per_s_kernel": round(nh / mk * 1e3), "hits_per_s_library": round(nh / ml * 1e3),
               "reads_per_s_library": round(args.reads / ml * 1e3), "library_over_count": round(ml / count_ms, 2),
               "steps_per_read": round(st["steps"] / args.reads, 1), "lines_per_read": round(st["line_reads"] / args.reads, 1),
               "busy": round(st["steps"] / max(st["wave_steps"], 1), 3), "batches": st["batches"],
               "launches": st["launches"], "scratch_GB": round(st["scratch_bytes"] / 1e9, 2)}
        res["runs"].append(row)
        print(json.dumps(row), flush=True)
    fm.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as out:
        out.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
