"""Suffix-prefix overlaps with mismatches on one GPU (debwt_fm_overlaps_mm) beside the exact debwt_fm_overlaps on the same
reads and index, written to a profile.

    python scripts/gpu_fm_overlap_mm_bench.py --out profiles/r14_fm_overlaps_mm.txt

The read set of scripts/gpu_fm_overlap_bench.py (same seed: `reads` reads of `length` bases at uniform positions of a
random genome of reads x length / coverage bases, forward strand only), once as it is and once with every base
substituted with probability --error (always by another base; its own seed).  Each set is indexed at s = 32 and queried
against its own index at min_overlap (default 40): the exact call as the yardstick, then the new call at K = 0, 1, 2 and
at K = 2 with 50 permille.  Every library call is made directly with a buffer of the known size (one call, no
DEBWT_ERANGE round), --reps times after one untimed call of the same shape; every list is [median, smallest, largest].
ms_kernel: the launches by events; ms_library: host time of the call (upload, launches, the runs' download and order on
the host, the expansion's download, the sort by record inside equal lengths).  busy = rank steps / wave steps.  At K = 0
the hits are compared with the exact call's, byte for byte."""
import argparse
import ctypes
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
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_overlaps_mm.txt"))
    args = ap.parse_args()
    from debwt_amd import _lib, api
    L = _lib.lib()
    rng = np.random.default_rng(1)
    G = int(args.reads * args.length / args.coverage)
    genome = rng.integers(0, 4, G).astype(np.uint8)          # codes; the same draws as gpu_fm_overlap_bench.py
    starts = rng.integers(0, G - args.length + 1, args.reads)
    clean = genome[(starts[:, None] + np.arange(args.length)[None, :])]
    rng2 = np.random.default_rng(2)
    flip = rng2.random(clean.shape, dtype=np.float32) < args.error
    noisy = np.where(flip, (clean + rng2.integers(1, 4, clean.shape, dtype=np.uint8)) % 4, clean).astype(np.uint8)
    offs = np.arange(args.reads + 1, dtype=np.uint64) * np.uint64(args.length)
    hoff = np.zeros(args.reads + 1, dtype=np.uint64)
    hp = ctypes.POINTER(_lib.DebwtFmOverlap)

    def spread(v):
        return [round(float(np.median(v)), 2), round(float(min(v)), 2), round(float(max(v)), 2)]

    for name, codes in (("clean", clean), ("error %g" % args.error, noisy)):
        buf = np.frombuffer(b"ACGT", dtype=np.uint8)[codes.ravel()].tobytes()
        rs = [buf[i * args.length:(i + 1) * args.length] for i in range(args.reads)]
        d = api.DeBWT(k=32)
        d.load_ascii(rs)
        d.build()
        fm = d.fm_index(sa_sample=32)
        d.close()
        res = {"set": name, "reads": args.reads, "length": args.length, "coverage": args.coverage, "genome": G, "n": fm.n,
               "min_overlap": args.min_overlap, "substituted_bases": int(flip.sum()) if codes is noisy else 0, "runs": []}
        exact = fm.overlaps(rs, min_overlap=args.min_overlap)          # also the record table and the scratch
        total = len(exact.all_hits)
        hits = np.zeros(max(total, 1), dtype=api._OVERLAP_DTYPE)
        kern, lib = [], []
        for _ in range(args.reps):
            rc = L.debwt_fm_overlaps(fm._h, buf, api._p64(offs), args.reads, args.min_overlap, 0, api._p64(hoff),
                                     hits.ctypes.data_as(hp), total)
            assert rc == 0
            st = fm.overlaps_stats()
            kern.append(st["ms_kernel"]); lib.append(st["ms_wall"])
        exact_ms = float(np.median(lib))
        res["exact"] = {"ms_kernel": spread(kern), "ms_library": spread(lib), "hits": total, "runs": st["runs"],
                        "lines_per_read": round(st["line_reads"] / args.reads, 1),
                        "busy": round(st["steps"] / max(st["wave_steps"], 1), 3)}
        print(json.dumps({"set": name, "exact": res["exact"]}), flush=True)
        base_hits = None
        for K, permille in ((0, 0), (1, 0), (2, 0), (2, 50)):
            t0 = time.perf_counter()
            r = fm.overlaps_mm(rs, min_overlap=args.min_overlap, mismatches=K, error_permille=permille)   # untimed; the count
            first_s = time.perf_counter() - t0
            nh = len(r.all_hits)
            if K == 0:
                assert np.array_equal(r.offsets, exact.offsets) and np.array_equal(r.all_hits, exact.all_hits)
                base_hits = nh
            by_mm = np.bincount(r.mismatches(), minlength=K + 1).tolist()
            del r
            hits = np.zeros(max(nh, 1), dtype=api._OVERLAP_DTYPE)
            kern, lib = [], []
            for _ in range(args.reps):
                rc = L.debwt_fm_overlaps_mm(fm._h, buf, api._p64(offs), args.reads, args.min_overlap, K, permille, 0,
                                            api._p64(hoff), hits.ctypes.data_as(hp), nh)
                assert rc == 0 and int(hoff[-1]) == nh
                st = fm.overlaps_mm_stats()
                kern.append(st["ms_kernel"]); lib.append(st["ms_wall"])
            ml = float(np.median(lib))
            row = {"K": K, "permille": permille, "reps": args.reps, "ms_kernel": spread(kern), "ms_library": spread(lib),
                   "library_over_exact": round(ml / exact_ms, 2), "hits": nh, "hits_by_mm": by_mm,
                   "hits_over_K0": round(nh / max(base_hits, 1), 3), "runs": st["runs"], "items": st["items"],
                   "retries": st["retries"], "launches": st["launches"], "batches": st["batches"],
                   "busy": round(st["steps"] / max(st["wave_steps"], 1), 3),
                   "steps_per_read": round(st["steps"] / args.reads, 1), "lines_per_read": round(st["line_reads"] / args.reads, 1),
                   "scratch_GB": round(st["scratch_bytes"] / 1e9, 2), "first_call_s": round(first_s, 2)}
            res["runs"].append(row)
            print(json.dumps(row), flush=True)
        del exact
        fm.close()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as out:
            out.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
