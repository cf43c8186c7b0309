"""Gapped extension and the read mapper on one GPU (debwt_fm_extend, debwt_fm_map), written to a profile.

    python scripts/gpu_fm_map_bench.py --workloads pan1x3.1G --out profiles/r10_fm_map.txt

Per workload: build the BWT, make the index at s = 32, attach the text, draw --reads reads of --length bases from the
text with --edits of their bases edited (substitutions, and 1-3 b insertions and deletions), half of them reverse
complemented.  Then, warm, --runs times each (median, min and max reported):
  * FMIndex.map with the defaults: wall time and its split over MEMs / locate / candidates / extension;
  * FMIndex.extend of the jobs the mapper extended (the winner of every mapped read) at w = 8, 16, 32, with and without
    the traceback: kernel ms (events), cells per second, lanes busy = cells / (64 x wave steps);
  * FMIndex.mems forward and both strands, to set beside profiles/r09_fm_mems.txt in the same session.
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


def edit(pats, share, rng):
    """each read with ~share of its bases edited: substitution, or an insertion / deletion of 1-3 bases"""
    out = []
    for k, p in enumerate(pats):
        b = bytearray(p)
        for _ in range(int(rng.binomial(len(b), share))):
            j = int(rng.integers(1, len(b) - 4))
            kind = int(rng.integers(0, 4))
            L = int(rng.integers(1, 4))
            if kind < 2:
                b[j] = b"ACGT"[int(rng.integers(0, 4))]
            elif kind == 2:
                b[j:j] = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, L))
            else:
                del b[j:j + L]
        p = bytes(b)
        out.append(p.translate(COMP)[::-1] if k % 2 else p)
    return out


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}


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
    fm.attach_text(d)
    d.close()
    rng = np.random.default_rng(1)
    rs = edit(draw(text.a, sep, n, args.length, args.reads, rng, mutate=0.0), args.edits, rng)
    res = {"workload": name, "n": n, "nrec": nrec, "reads": len(rs), "length": args.length, "edits": args.edits,
           "runs": args.runs}
    fm.map(rs[:1000])                                             # scratch allocated outside the timing
    walls, stages = [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        mr = fm.map(rs)
        walls.append(time.perf_counter() - t0)
        stages.append(fm.map_stats())
    st = stages[-1]
    res["map"] = {"wall_s": spread(walls), "mapped": st["mapped"], "seeds": st["seeds"], "jobs": st["jobs"],
                  **{k: spread([s[k] for s in stages]) for k in ("ms_mems", "ms_locate", "ms_candidates", "ms_extend")}}
    print(json.dumps(res["map"]), flush=True)
    ok = np.nonzero(mr.mapped)[0]
    jobs = [(int(i), int(mr.strand[i]), int(mr.diag[i]), int(mr.record[i])) for i in ok]
    res["extend"] = []
    for w in (8, 16, 32):
        for cigar in (True, False):
            fm.extend(rs, jobs[:1000], band=w, cigar=cigar)
            ms, tr, cells, steps = [], [], 0, 1
            for _ in range(args.runs):
                fm.extend(rs, jobs, band=w, cigar=cigar)
                xs = fm.extend_stats()
                ms.append(xs["ms_kernel"])
                tr.append(xs["ms_trace"])
                cells, steps = xs["cells"], xs["wave_steps"]
            row = {"w": w, "traceback": cigar, "jobs": len(jobs), "ms_kernel": spread(ms), "ms_trace": spread(tr),
                   "gcups": round(cells / (sorted(ms)[len(ms) // 2] * 1e6), 2), "busy": round(cells / (64 * steps), 3),
                   "batches": xs["batches"], "scratch_GB": round(xs["scratch_bytes"] / 1e9, 2)}
            res["extend"].append(row)
            print(json.dumps(row), flush=True)
    res["mems"] = []
    for strands in ("forward", "both"):
        fm.mems(rs[:1000], strands=strands)
        ms, walls = [], []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            fm.mems(rs, strands=strands)
            walls.append(time.perf_counter() - t0)
            ms.append(fm.mems_stats()["ms_kernel"])
        res["mems"].append({"strands": strands, "ms_kernel": spread(ms), "wall_s": spread(walls)})
        print(json.dumps(res["mems"][-1]), flush=True)
    fm.close()
    text.free()
    syn.close()
    with open(out, "a") as f:
        f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pan1x3.1G")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--edits", type=float, default=0.02)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_map.txt"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        run(args.child, args, args.out)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.workloads.split(","):                        # a fresh process per workload; a failure ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reads", str(args.reads), "--length",
               str(args.length), "--edits", str(args.edits), "--runs", str(args.runs), "--out", args.out]
        rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        if rc:
            sys.exit(f"{name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
