"""Pileup and calls on one GPU (debwt_fm_pileup, debwt_fm_pile_call) beside the debwt_fm_map call that made the
alignments, written to a profile.

    python scripts/gpu_fm_pileup_bench.py --out profiles/r23_fm_pileup.txt

The read set of scripts/gpu_fm_overlap_mm_bench.py with 1 % substitutions (same seeds: `reads` reads of `length` bases at
uniform positions of a random genome of reads x length / coverage bases), mapped back to the genome they were sampled
from (one record, s = 32, the mapper's defaults).  The mapped hits are piled up over the whole text by each counting form
(DEBWT_PILE_FORM = lane, group16, group64) and called with the defaults; every timed call runs --reps times after one
untimed call of the same shape and every list is [median, smallest, largest].  ms_kernel: the counting kernel by events;
ms_plan: the validity pass; ms_library: host time of the call (uploads, staging, launches).  The tables of the forms are
compared with each other and with the same counts made on the host by numpy (the loop of tests/pileup_ref.py restated
over arrays), whose time is the CPU figure.  The substitutions are per-read errors, not variants, so the calls should
find almost nothing: the number is reported."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_counts(codes, length, rows, coff, cg, n, chunk=100_000):
    """definition 7 over the whole text with numpy: the ops of a chunk of alignments expanded to columns, one bincount"""
    table = np.zeros(n * 8, dtype=np.int64)
    for a in range(0, len(rows), chunk):
        b = min(a + chunk, len(rows))
        ops = cg[int(coff[a]):int(coff[b])].astype(np.int64)
        kind, ln = ops & 15, ops >> 4
        nops = (coff[a + 1:b + 1] - coff[a:b]).astype(np.int64)
        owner = np.repeat(np.arange(a, b), nops)
        first = (coff[a:b] - coff[a]).astype(np.int64)[nops > 0]
        ql, tl = np.where(kind != 2, ln, 0), np.where(kind != 1, ln, 0)
        qs, ts = np.cumsum(ql) - ql, np.cumsum(tl) - tl        # running sums, rebased at the first op of every alignment
        qs -= np.repeat(qs[first], nops[nops > 0])
        ts -= np.repeat(ts[first], nops[nops > 0])
        qs += rows["qbeg"][owner].astype(np.int64)
        ts += rows["tbeg"][owner].astype(np.int64)
        for k, slot in ((0, None), (2, 4)):
            sel = kind == k
            reps = ln[sel]
            col = np.arange(int(reps.sum())) - np.repeat(np.cumsum(reps) - reps, reps)
            t = np.repeat(ts[sel], reps) + col
            if slot is None:
                own = np.repeat(owner[sel], reps)
                q = np.repeat(qs[sel], reps) + col
                rev = rows["strand"][own] == 1
                c = codes[rows["pattern"][own].astype(np.int64) * length + np.where(rev, length - 1 - q, q)].astype(np.int64)
                s = np.where(rev, 3 - c, c)
            else:
                s = slot
            table += np.bincount(t * 8 + s, minlength=n * 8)
        sel = kind == 1
        table += np.bincount((ts[sel] - 1) * 8 + 5, minlength=n * 8)
    return table.reshape(n, 8).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_pileup.txt"))
    args = ap.parse_args()
    from debwt_amd import api
    rng = np.random.default_rng(1)
    G = int(args.reads * args.length / args.coverage)
    genome = rng.integers(0, 4, G).astype(np.uint8)          # codes; the same draws as gpu_fm_overlap_bench.py
    starts = rng.integers(0, G - args.length + 1, args.reads)
    clean = genome[(starts[:, None] + np.arange(args.length)[None, :])]
    rng2 = np.random.default_rng(2)
    flip = rng2.random(clean.shape, dtype=np.float32) < args.error
    noisy = np.where(flip, (clean + rng2.integers(1, 4, clean.shape, dtype=np.uint8)) % 4, clean).astype(np.uint8)
    buf = np.frombuffer(b"ACGT", dtype=np.uint8)[noisy.ravel()].tobytes()
    offs = np.arange(args.reads + 1, dtype=np.uint64) * np.uint64(args.length)
    reads = (buf, offs)

    def spread(v):
        return [round(float(np.median(v)), 3), round(float(min(v)), 3), round(float(max(v)), 3)]

    d = api.DeBWT(k=32)
    d.load_records([genome])
    d.build()
    fm = d.fm_index(sa_sample=32)
    fm.attach_text(d)
    d.close()
    res = {"reads": args.reads, "length": args.length, "coverage": args.coverage, "genome": G, "n": fm.n,
           "substituted_bases": int(flip.sum())}
    fm.map(reads)                                             # untimed: scratch of the mapper
    lib = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        mp = fm.map(reads)
        lib.append((time.perf_counter() - t0) * 1e3)
    ms = fm.map_stats()
    res["map"] = {"ms_call": spread(lib), "ms_library": round(ms["ms_wall"], 2), "mapped": int(mp.mapped.sum())}
    alns = mp.alignments(0)
    rows, coff, cg = alns
    res["alignments"] = len(rows)
    tables = {}
    for form in ("lane", "group16", "group64"):
        os.environ["DEBWT_PILE_FORM"] = form
        fm.pileup(reads, alns)
        kern, plan, wall = [], [], []
        for _ in range(args.reps):
            r = fm.pileup(reads, alns)
            st = fm.pile_stats()
            kern.append(st["ms_kernel"]); plan.append(st["ms_plan"]); wall.append(st["ms_wall"])
        tables[form] = r.counts
        res[form] = {"ms_kernel": spread(kern), "ms_plan": spread(plan), "ms_library": spread(wall),
                     "events_per_s": round((st["ev_base"] + st["ev_other"] + st["ev_del"] + st["ev_ins"]) / np.median(kern) * 1e3)}
        res["events"] = {k: st[k] for k in ("ops", "m_columns", "d_bases", "i_ops", "ev_base", "ev_other", "ev_del", "ev_ins")}
        print(json.dumps({form: res[form]}), flush=True)
    del os.environ["DEBWT_PILE_FORM"]
    res["forms_agree"] = bool(np.array_equal(tables["lane"], tables["group16"]) and np.array_equal(tables["lane"], tables["group64"]))
    fm.pileup(reads, alns)
    res["default_group"] = fm.pile_stats()["group"]
    fm.pile_call()
    kern, wall = [], []
    for _ in range(args.reps):
        calls, ref, var = fm.pile_call()
        st = fm.pile_stats()
        kern.append(st["ms_call"]); wall.append(st["ms_call_wall"])
    res["call"] = {"ms_kernel": spread(kern), "ms_library": spread(wall), "variants": len(var),
                   "called": int((calls != api.PILE_NO_CALL).sum()), "positions": len(calls)}
    res["pileup_plus_call_ms_library"] = round(res["group%d" % res["default_group"]]["ms_library"][0] + res["call"]["ms_library"][0], 2)
    t0 = time.perf_counter()
    host = host_counts(noisy.ravel(), args.length, rows, coff, cg, fm.n)
    res["host_numpy"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "equal": bool(np.array_equal(host, tables["lane"]))}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
