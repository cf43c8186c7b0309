"""Extension along a chain and the chained mapper on one GPU (debwt_fm_extend_chain, debwt_fm_map_chained), written to a
profile.

    python scripts/gpu_fm_chain_bench.py --workloads pan1x3.1G --out profiles/r11_fm_chain.txt

Per workload: build the BWT, make the index at s = 32, attach the text.  Then, warm, --runs times each (median, min and
max reported):
  (a) one-anchor jobs through FMIndex.extend_chain against the same jobs through FMIndex.extend -- the fixed-band kernel,
      which this library carries unchanged --: --short-jobs jobs of 150 b and --long-jobs jobs of 10 kb at their true
      diagonal, w = 16 and w = 63, with and without the traceback: kernel ms (events) of both and their ratio;
  (b) lanes busy of both from the statistics: cells / (64 x wave steps), a wave step being an anti-diagonal of the fixed
      band and a query row of the chain sweep (which holds up to two band indices per lane above w = 31);
  (c) FMIndex.map_chained on --reads simulated reads of --length bases (--edits of their bases edited, plus --indels
      indels of 10-40 b of one sign per read): wall time and its split over MEMs / locate / chaining / extension.
Every workload runs in a child process of its own under --step-timeout seconds; the first failure ends the script."""
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


def drift(pats, indels, rng):
    """each read with `indels` insertions or deletions (one sign per read) of 10-40 bases, at least 100 bases apart"""
    out = []
    for p in pats:
        b = bytearray(p)
        ins = bool(rng.integers(0, 2))
        slots = sorted((int(x) for x in rng.choice(np.arange(1, max(len(b) // 100 - 1, 2)), size=min(indels, max(len(b) // 100 - 2, 1)),
                                                   replace=False)), reverse=True)
        for s in slots:
            n = int(rng.integers(10, 41))
            if ins:
                b[100 * s:100 * s] = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, n))
            else:
                del b[100 * s:100 * s + n]
        out.append(bytes(b))
    return out


def run(name, args, out):
    from debwt_amd import api
    from debwt_amd import synth_native as SN
    from gpu_fm_bench import draw
    from gpu_fm_map_bench import edit, spread
    syn = SN.Synth.named(name)
    n, nrec = syn.n, syn.nrec
    sep = np.asarray(syn.sep(), dtype=np.int64)
    text = SN.PinnedArray(syn.nwords)
    syn.words_into(text.ptr)
    d = api.DeBWT(k=32)
    d.load_packed(text.a, n, sep.astype(np.uint64))
    d.build()
    fm = d.fm_index(sa_sample=32)
    fm.attach_text(d)
    d.close()
    rng = np.random.default_rng(1)
    res = {"workload": name, "n": n, "nrec": nrec, "runs": args.runs, "one_anchor": []}
    # (a), (b): error-free reads at their true locus, found by the plain mapper
    for length, count in ((150, args.short_jobs), (10_000, args.long_jobs)):
        rs = draw(text.a, sep, n, length, count, rng, mutate=0.0)
        mr = fm.map(rs, max_cand=1)
        ok = np.nonzero(mr.mapped)[0]
        jobs = [(int(i), int(mr.strand[i]), int(mr.diag[i]), int(mr.record[i])) for i in ok]
        cj = [(p, s, r, k, 1) for k, (p, s, dg, r) in enumerate(jobs)]
        ca = [(0, dg) for _, _, dg, _ in jobs]
        for w in (16, 63):
            for cigar in (True, False):
                row = {"length": length, "jobs": len(jobs), "w": w, "traceback": cigar}
                for key, call in (("extend", lambda: fm.extend(rs, jobs, band=w, cigar=cigar)),
                                  ("chain", lambda: fm.extend_chain(rs, cj, ca, band=w, cigar=cigar))):
                    call()
                    ms, tr = [], []
                    for _ in range(args.runs):
                        call()
                        xs = fm.extend_stats()
                        ms.append(xs["ms_kernel"])
                        tr.append(xs["ms_trace"])
                    row[key] = {"ms_kernel": spread(ms), "ms_trace": spread(tr), "cells": xs["cells"], "wave_steps": xs["wave_steps"],
                                "busy": round(xs["cells"] / (64 * xs["wave_steps"]), 3),
                                "gcups": round(xs["cells"] / (sorted(ms)[len(ms) // 2] * 1e6), 2)}
                row["chain_over_extend"] = round(row["chain"]["ms_kernel"]["median"] / row["extend"]["ms_kernel"]["median"], 2)
                res["one_anchor"].append(row)
                print(json.dumps(row), flush=True)
    # (c): the stage split of the chained mapper
    rs = drift(edit(draw(text.a, sep, n, args.length, args.reads, rng, mutate=0.0), args.edits, rng), args.indels, rng)
    fm.map_chained(rs[:100], band=args.band)
    walls, stages = [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        mr = fm.map_chained(rs, band=args.band)
        walls.append(time.perf_counter() - t0)
        stages.append(fm.map_stats())
    st = stages[-1]
    full = int(((mr.qend.astype(np.int64) - mr.qbeg) >= 0.9 * np.array([len(r) for r in rs])).sum())
    res["map_chained"] = {"reads": len(rs), "length": args.length, "band": args.band, "wall_s": spread(walls),
                          "mapped": st["mapped"], "aligned_over_90_percent": full, "seeds": st["seeds"], "chains": st["jobs"],
                          **{k: spread([s[k] for s in stages]) for k in ("ms_mems", "ms_locate", "ms_candidates", "ms_extend")}}
    print(json.dumps(res["map_chained"]), flush=True)
    fm.close()
    text.free()
    syn.close()
    with open(out, "a") as f:
        f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pan1x3.1G")
    ap.add_argument("--short-jobs", type=int, default=100_000)
    ap.add_argument("--long-jobs", type=int, default=1_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--length", type=int, default=10_000)
    ap.add_argument("--edits", type=float, default=0.01)
    ap.add_argument("--indels", type=int, default=8)
    ap.add_argument("--band", type=int, default=63)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_chain.txt"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        run(args.child, args, args.out)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.workloads.split(","):                        # a fresh process per workload; a failure ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out]
        for k in ("short_jobs", "long_jobs", "reads", "length", "edits", "indels", "band", "runs"):
            cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
        rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        if rc:
            sys.exit(f"{name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
