"""The k-mer spectrum of the indexed collection (debwt_fm_spectrum, debwt_fm_kmer_list) on one GPU, written to a profile.

    python scripts/gpu_fm_spectrum_bench.py --out profiles/r24_fm_spectrum.txt

The read set of scripts/gpu_fm_kmer_bench.py (same seeds: `reads` reads of `length` bases at uniform positions of a random
genome of reads x length / coverage bases, forward strand only, every base substituted with probability --error), indexed
at s = 32.  Per k in --k, in a child process of its own under --step-timeout seconds (the first failure ends the script),
and per strand setting (both, forward):

spectrum  one untimed call (it builds the table and the scratch), then --reps timed calls of debwt_fm_spectrum with 256
          bins: ms_kernel (events, first chunk to last kernel), ms_library (host time of the call), the statistics of the
          last call (busy = rank steps / wave steps, the intervals of every depth, look-ups), valley, peak and est_size.
items     the same call at DEBWT_FM_SPECTRUM_ITEMS = 2^18, 2^20, 2^24 (the default is 2^22): ms_kernel, chunks, scratch.
list      debwt_fm_kmer_list of the solid k-mers (multiplicity >= valley): the sizing call and the filling call, with
          the host sort inside the second.
route     today's route to the same histogram, in the same process so its repeats alternate with the spectrum's:
          debwt_fm_kmer_counts of all reads on the same strands, then numpy: every k-mer instance of count c weighs 1 / c
          (both strands: 2 / c for a k-mer that is its own reverse complement), binned by min(c, 255).  The histogram
          is compared with the spectrum's, bin by bin (equal up to the rounding of the weights' sum).
Every list is [median, smallest, largest]."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return [round(float(np.median(v)), 2), round(float(min(v)), 2), round(float(max(v)), 2)]


def run(k, args):
    from debwt_amd import _lib, api
    L = _lib.lib()
    rng = np.random.default_rng(1)
    n, m = args.reads, args.length
    G = int(n * m / args.coverage)
    genome = rng.integers(0, 4, G).astype(np.uint8)          # codes; the same draws as gpu_fm_kmer_bench.py
    starts = rng.integers(0, G - m + 1, n)
    clean = genome[(starts[:, None] + np.arange(m)[None, :])]
    rng2 = np.random.default_rng(2)
    flip = rng2.random(clean.shape, dtype=np.float32) < args.error
    noisy = np.where(flip, (clean + rng2.integers(1, 4, clean.shape, dtype=np.uint8)) % 4, clean).astype(np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[noisy]
    buf = letters.tobytes()
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(m)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    d = api.DeBWT(k=32)
    t0 = time.perf_counter()
    d.load_ascii([buf[i * m:(i + 1) * m] for i in range(n)])
    d.build()
    fm = d.fm_index(sa_sample=32)
    d.close()
    head = {"reads": n, "length": m, "coverage": args.coverage, "genome": G, "error": args.error, "n": fm.n,
            "index_build_s": round(time.perf_counter() - t0, 2), "k": k, "bins": 256}
    nk = m - k + 1
    total = n * nk
    hist = np.zeros(256, dtype=np.uint64)
    tot = _lib.DebwtFmSpectrumTotals()

    def spectrum(flags):
        rc = L.debwt_fm_spectrum(fm._h, k, flags, 256, api._p64(hist), ctypes.byref(tot))
        assert rc == 0, L.debwt_fm_last_error(fm._h)
        return fm.spectrum_stats()

    if args.route:                                                # own reverse complement, per k-mer instance (even k only)
        win = np.lib.stride_tricks.sliding_window_view(noisy, k, axis=1)
        selfrc = (win == 3 - win[:, :, ::-1]).all(axis=2).reshape(-1) if k % 2 == 0 else None
        coff = np.zeros(n + 1, dtype=np.uint64)
        counts = np.zeros(total, dtype=np.uint32)
    for name, flags in (("both", 1), ("forward", 0)):
        os.environ.pop("DEBWT_FM_SPECTRUM_ITEMS", None)
        first = spectrum(flags)
        kern, lib, route, route_counts = [], [], [], []
        for _ in range(args.reps):
            st = spectrum(flags)
            assert st["ms_table"] == 0
            kern.append(st["ms_kernel"]); lib.append(st["ms_wall"])
            if args.route:
                t0 = time.perf_counter()
                rc = L.debwt_fm_kmer_counts(fm._h, buf, api._p64(offs), n, k, flags, api._p64(coff), counts.ctypes.data_as(u32p), total)
                assert rc == 0
                t1 = time.perf_counter()
                w = 1.0 / counts
                if flags and selfrc is not None:
                    w[selfrc] *= 2
                rh = np.bincount(np.minimum(counts, 255), weights=w, minlength=256)
                route.append((time.perf_counter() - t0) * 1e3); route_counts.append((t1 - t0) * 1e3)
        h = hist.copy()
        summary = api.spectrum_threshold(h, tot.total)
        row = {**head, "part": "spectrum", "strands": name, "reps": args.reps, "ms_kernel": spread(kern), "ms_library": spread(lib),
               "ms_table": round(first["ms_table"], 2), "distinct": int(tot.distinct), "total": int(tot.total),
               "overflow_total": int(tot.overflow_total), **summary, "est_size_over_genome": round(summary["est_size"] / G, 4),
               "hist_1_to_40": [int(x) for x in h[1:41]], "chunks": st["chunks"], "launches": st["launches"],
               "levels": st["levels"], "expanded": st["expanded"], "leaves": st["leaves"], "lookups": st["lookups"],
               "steps": st["steps"], "line_reads": st["line_reads"], "busy": round(st["steps"] / max(st["wave_steps"], 1), 3),
               "intervals_per_level": {str(dd): v for dd, v in enumerate(st["level_intervals"]) if v},
               "items_limit": st["items_limit"], "scratch_MB": round(st["scratch_bytes"] / 1e6, 1), "table_q": st["table_q"]}
        if args.route:
            # the last bin of the route holds instances / c with c >= 255, not distinct k-mers of 255 and more: leave it out
            diff = float(np.abs(rh[1:255] - h[1:255].astype(np.float64)).max())
            row.update({"route_ms": spread(route), "route_ms_kmer_counts": spread(route_counts), "route_kmer_instances": total,
                        "route_max_bin_difference": round(diff, 3)})
            assert diff < 0.5, diff
        emit(args, row)
        rows = []
        for items in (1 << 18, 1 << 20, 1 << 24):
            os.environ["DEBWT_FM_SPECTRUM_ITEMS"] = str(items)
            spectrum(flags)
            ks = []
            for _ in range(3):
                st = spectrum(flags)
                ks.append(st["ms_kernel"])
            assert np.array_equal(hist, h)
            rows.append({"items": items, "ms_kernel": spread(ks), "chunks": st["chunks"], "scratch_MB": round(st["scratch_bytes"] / 1e6, 1)})
        os.environ.pop("DEBWT_FM_SPECTRUM_ITEMS", None)
        emit(args, {"part": "items", "k": k, "strands": name, "rows": rows})
        lo = max(summary["valley"], 1)
        cnt = ctypes.c_uint64(0)
        t0 = time.perf_counter()
        rc = L.debwt_fm_kmer_list(fm._h, k, flags, lo, 2 ** 32 - 1, None, None, 0, ctypes.byref(cnt))
        assert rc in (0, -5)
        t1 = time.perf_counter()
        codes = np.zeros(max(cnt.value, 1), dtype=np.uint64)
        mults = np.zeros(max(cnt.value, 1), dtype=np.uint32)
        rc = L.debwt_fm_kmer_list(fm._h, k, flags, lo, 2 ** 32 - 1, api._p64(codes), mults.ctypes.data_as(u32p), cnt.value, ctypes.byref(cnt))
        assert rc == 0
        t2 = time.perf_counter()
        st = fm.spectrum_stats()
        assert bool((codes[1:cnt.value] > codes[:cnt.value - 1]).all()) and cnt.value == int(h[lo:].sum())
        emit(args, {"part": "list", "k": k, "strands": name, "at_least": lo, "members": cnt.value,
                    "ms_sizing_call": round((t1 - t0) * 1e3, 2), "ms_filling_call": round((t2 - t1) * 1e3, 2),
                    "ms_kernel_and_staging": round(st["ms_kernel"], 2), "scratch_MB": round(st["scratch_bytes"] / 1e6, 1)})
    fm.close()


def emit(args, row):
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as out:
        out.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--k", type=int, nargs="+", default=[21, 31])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-route", dest="route", action="store_false")
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_spectrum.txt"))
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        run(args.child, args)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for k in args.k:                                              # a fresh process per k; a failure ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(k), "--out", args.out, "--reads", str(args.reads),
               "--length", str(args.length), "--coverage", str(args.coverage), "--error", str(args.error), "--reps", str(args.reps)]
        if not args.route:
            cmd.append("--no-route")
        rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        if rc:
            sys.exit(f"k = {k}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
