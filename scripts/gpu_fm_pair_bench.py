"""Alignment in a text window and the paired-end mapper on one GPU (debwt_fm_align_window, debwt_fm_map_pairs), written to
a profile.

    python scripts/gpu_fm_pair_bench.py --workloads pan1x3.1G --out profiles/r12_fm_pairs.txt

Per workload: build the BWT, make the index at s = 32, attach the text.  Then, warm, --runs times each (median, min and
max reported):
  (a) FMIndex.align_window on --jobs jobs of 150 x 600 and of 250 x 1500 (a read cut from the text with 2 % of its bases
      substituted, half of them reverse complemented, against a window that holds its origin at a random offset), with and
      without the traceback: kernel ms (events), cells per second, lanes busy = cells / (64 x wave steps); beside it
      FMIndex.extend at w = 16 on the same reads at their true diagonal, for scale;
  (b) FMIndex.map_pairs on --pairs pairs of 2 x 150 b (template length 300..500, every fifth mate 2 with a substitution
      at every 16th base, so that it has no seed and is rescued): wall time and its split over candidates / rescue /
      selection, proper pairs, rescue jobs, rescued mates, the estimated insert bounds.
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
COMP = bytes.maketrans(b"ACGT", b"TGCA")
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}


def cut(words, sep, n, L, count, rng):
    """count stretches of L bases at random text positions that cross no separator: (positions, records, codes)"""
    pos = rng.integers(0, n - L, size=count * 2, dtype=np.int64)
    rec = np.searchsorted(sep, pos)
    ok = rec == np.searchsorted(sep, pos + L)
    pos, rec = pos[ok][:count], rec[ok][:count]
    idx = pos[:, None] + np.arange(L)[None, :]
    codes = ((words[idx >> 5] >> (2 * (31 - (idx & 31))).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)
    return pos, rec, codes


def substituted(codes, share, rng):
    c = codes.copy()
    hit = rng.random(c.shape) < share
    c[hit] = (c[hit] + rng.integers(1, 4, size=int(hit.sum())).astype(np.uint8)) & 3
    return c


def as_reads(codes, reverse):
    out = [bytes(r) for r in LETTERS[codes]]
    return [p.translate(COMP)[::-1] if rv else p for p, rv in zip(out, reverse)]


def window_rows(fm, words, sep, n, m, L, count, runs, rng):
    pos, rec, codes = cut(words, sep, n, m, count, rng)
    strand = (np.arange(len(pos)) % 2).astype(np.int64)
    reads = as_reads(substituted(codes, 0.02, rng), strand)
    wbeg = np.maximum(pos - rng.integers(0, L - m + 1, size=len(pos)), 0)
    jobs = [(k, int(strand[k]), int(rec[k]), int(wbeg[k]), int(wbeg[k]) + L) for k in range(len(pos))]
    rows = []
    for cigar in (False, True):
        fm.align_window(reads[:1000], jobs[:1000], cigar=cigar)    # scratch allocated outside the timing
        ms, tr = [], []
        for _ in range(runs):
            fm.align_window(reads, jobs, cigar=cigar)
            xs = fm.extend_stats()
            ms.append(xs["ms_kernel"])
            tr.append(xs["ms_trace"])
        rows.append({"kernel": "k_fm_window", "m": m, "window": L, "traceback": cigar, "jobs": len(jobs),
                     "ms_kernel": spread(ms), "ms_trace": spread(tr), "cells": xs["cells"],
                     "gcups": round(xs["cells"] / (sorted(ms)[len(ms) // 2] * 1e6), 2),
                     "busy": round(xs["cells"] / (64 * xs["wave_steps"]), 3), "batches": xs["batches"],
                     "scratch_GB": round(xs["scratch_bytes"] / 1e9, 2)})
        print(json.dumps(rows[-1]), flush=True)
    xjobs = [(k, int(strand[k]), int(pos[k]), int(rec[k])) for k in range(len(pos))]
    for cigar in (False, True):
        fm.extend(reads[:1000], xjobs[:1000], band=16, cigar=cigar)
        ms = []
        for _ in range(runs):
            fm.extend(reads, xjobs, band=16, cigar=cigar)
            xs = fm.extend_stats()
            ms.append(xs["ms_kernel"])
        rows.append({"kernel": "k_fm_extend", "m": m, "w": 16, "traceback": cigar, "jobs": len(xjobs), "ms_kernel": spread(ms),
                     "cells": xs["cells"], "gcups": round(xs["cells"] / (sorted(ms)[len(ms) // 2] * 1e6), 2),
                     "busy": round(xs["cells"] / (64 * xs["wave_steps"]), 3)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def run(name, args, out):
    from debwt_amd import api
    from debwt_amd import synth_native as SN
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
    res = {"workload": name, "n": n, "nrec": nrec, "runs": args.runs, "window": []}
    for m, L in ((150, 600), (250, 1500)):
        res["window"] += window_rows(fm, text.a, sep, n, m, L, args.jobs, args.runs, rng)
    # (b) pairs: a template of 300..500 bases, its first 150 and the reverse complement of its last 150
    pos, rec, codes = cut(text.a, sep, n, 500, args.pairs, rng)
    T = rng.integers(300, 501, size=len(pos))
    m1 = codes[:, :150]
    m2 = np.stack([codes[k, T[k] - 150:T[k]] for k in range(len(pos))])
    for k in range(4, len(pos), 5):                               # every fifth mate 2: a substitution at every 16th base
        j = np.arange(int(rng.integers(0, 16)), 150, 16)
        m2[k, j] = (m2[k, j] + 1) & 3
    r1 = as_reads(m1, np.zeros(len(pos), dtype=bool))
    r2 = as_reads(m2, np.ones(len(pos), dtype=bool))
    fm.map_pairs(r1[:1000], r2[:1000])
    walls, stats = [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        mr = fm.map_pairs(r1, r2)
        walls.append(time.perf_counter() - t0)
        stats.append(fm.pair_stats())
    st = stats[-1]
    res["pairs"] = {"pairs": st["pairs"], "length": 150, "wall_s": spread(walls), "mapped": int(mr.mapped.sum()),
                    "proper": st["proper"], "rescue_jobs": st["rescue_jobs"], "rescued": st["rescued"],
                    "ins_lo": st["ins_lo"], "ins_hi": st["ins_hi"], "estimate_pairs": st["estimate_pairs"],
                    **{k: spread([s[k] for s in stats]) for k in ("ms_candidates", "ms_rescue", "ms_select", "ms_wall")}}
    print(json.dumps(res["pairs"]), flush=True)
    fm.close()
    text.free()
    syn.close()
    with open(out, "a") as f:
        f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pan1x3.1G")
    ap.add_argument("--jobs", type=int, default=100_000)
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_pairs.txt"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        run(args.child, args, args.out)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.workloads.split(","):                        # a fresh process per workload; a failure ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--jobs", str(args.jobs), "--pairs", str(args.pairs),
               "--runs", str(args.runs), "--out", args.out]
        rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        if rc:
            sys.exit(f"{name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
