"""FM-index search with mismatches on one GPU (debwt_fm_search): kernel and wall time, items per level, rank lines per
pattern, written to a profile.

    python scripts/gpu_fm_search_bench.py --workloads pan1x3.1G --out profiles/r08_fm_search.txt

Per workload: build the BWT, make the index at s = 32, draw 10^6 patterns of 100 b from the text with 0..K random
substitutions (gpu_fm_bench.draw, then extra changes), and search them at K = 0, 1, 2 on the forward strand and on both.
ms_kernel sums the k_fm_search launches by events; wall_s is the host time of FMIndex.search (pattern upload, the
drains, the hit download and the per-pattern sort included).  K = 0 is reported next to FMIndex.ranges (count) on the
same patterns."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def mutate(pats, K, rng):
    """each pattern with 0..K random substitutions (uniform number, positions and letters)"""
    out = []
    for p in pats:
        b = bytearray(p)
        for _ in range(int(rng.integers(0, K + 1))):
            b[int(rng.integers(0, len(b)))] = b"ACGT"[int(rng.integers(0, 4))]
        out.append(bytes(b))
    return out


def run(name, args, out):
    from debwt_amd import api
    from debwt_amd import synth_native as SN
    from gpu_fm_bench import draw
    syn = SN.Synth.named(name)
    n, nrec = syn.n, syn.nrec
    sep = np.asarray(syn.sep(), dtype=np.int64)
    text = SN.PinnedArray(syn.nwords)
    syn.words_into(text.ptr)
    d = api.DeBWT(k=32)
    d.load_packed(text.a, n, sep.astype(np.uint64))
    d.build()
    fm = d.fm_index(sa_sample=32)
    d.close()
    rng = np.random.default_rng(1)
    base = draw(text.a, sep, n, args.length, args.patterns, rng, mutate=0.0)
    res = {"workload": name, "n": n, "nrec": nrec, "patterns": len(base), "length": args.length, "runs": []}
    fm.ranges(base[:1000])
    for K in (int(k) for k in args.k.split(",")):
        pats = mutate(base, K, rng)
        if K == 0:
            t0 = time.perf_counter()
            r = fm.ranges(pats)
            res["count_wall_s"] = round(time.perf_counter() - t0, 4)
            res["count_found"] = int((r[:, 1] > r[:, 0]).sum())
        for strands in ("forward", "both"):
            fm.search(pats[:1000], mismatches=K, strands=strands)        # scratch allocated outside the timing
            t0 = time.perf_counter()
            sr = fm.search(pats, mismatches=K, strands=strands)
            wall = time.perf_counter() - t0
            st = fm.search_stats()
            row = {"K": K, "strands": strands, "wall_s": round(wall, 4), "ms_kernel": round(st["ms_kernel"], 2),
                   "ms_library": round(st["ms_wall"], 2), "patterns_per_s": round(len(pats) / wall),
                   "items_per_level": st["items"][:K + 1], "hits": st["hits"],
                   "found": int((np.diff(sr.offsets) > 0).sum()), "steps_per_pattern": round(st["steps"] / len(pats), 1),
                   "lines_per_pattern": round(st["line_reads"] / len(pats), 1), "launches": st["launches"],
                   "retries": st["retries"], "scratch_GB": round(st["scratch_bytes"] / 1e9, 2)}
            res["runs"].append(row)
            print(json.dumps(row), flush=True)
    fm.close()
    text.free()
    syn.close()
    out.write(json.dumps(res) + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pan1x3.1G,pan10x3G")
    ap.add_argument("--patterns", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--k", default="0,1,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_search.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as out:
        for name in args.workloads.split(","):
            run(name, args, out)


if __name__ == "__main__":
    main()
