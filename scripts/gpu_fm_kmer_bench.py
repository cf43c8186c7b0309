"""k-mer counts along reads (debwt_fm_kmer_counts) and k-mer read correction (debwt_fm_correct) on one GPU, written to a
profile.

    python scripts/gpu_fm_kmer_bench.py --part profile  --out profiles/r18_fm_kmers.txt
    python scripts/gpu_fm_kmer_bench.py --part correct  --out profiles/r18_fm_kmers.txt
    python scripts/gpu_fm_kmer_bench.py --part overlaps --out profiles/r18_fm_kmers.txt

The read set of scripts/gpu_fm_overlap_mm_bench.py (same seeds: `reads` reads of `length` bases at uniform positions of a
random genome of reads x length / coverage bases, forward strand only, every base substituted with probability --error),
indexed at s = 32 and queried against its own index.  Every library call is made directly with buffers of the known
size; every list is [median, smallest, largest].

profile   per k in --k: the profile of all reads (forward strand) at DEBWT_FM_KMER_TABLE_Q = 0, 8, 10, 12 -- one untimed
          call per q, which builds the table (ms_table), then --reps timed calls -- and, after each q, one call of the
          yardstick: debwt_fm_count on the exploded k-mer list (the only way to the same numbers without the new call),
          so the yardstick's repeats alternate with the profile's.  The counts of every q are compared with the
          yardstick's ranges, all of them.  ms_kernel: the launches by events; ms_library: host time of the call
          without the table; busy = rank steps / wave steps.
correct   debwt_fm_correct at --correct-k, min_count 3, 4 rounds, both strands and forward only: time per round, the reads
          that got a fix per round, fixes, reads per flag, and the wrong bases before and after against the error-free
          reads.
overlaps  the exact overlaps of at least --min-overlap bases (debwt_fm_overlaps, forward) of the error-free reads, of the
          reads with errors and of the corrected reads, each against the index of its own set, with the time of
          correction + rebuild + overlaps."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return [round(float(np.median(v)), 2), round(float(min(v)), 2), round(float(max(v)), 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("profile", "correct", "overlaps"), required=True)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--k", type=int, nargs="+", default=[21, 31])
    ap.add_argument("--correct-k", type=int, default=21)
    ap.add_argument("--min-overlap", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_kmers.txt"))
    args = ap.parse_args()
    from debwt_amd import _lib, api
    L = _lib.lib()
    rng = np.random.default_rng(1)
    G = int(args.reads * args.length / args.coverage)
    genome = rng.integers(0, 4, G).astype(np.uint8)          # codes; the same draws as gpu_fm_overlap_mm_bench.py
    starts = rng.integers(0, G - args.length + 1, args.reads)
    clean = genome[(starts[:, None] + np.arange(args.length)[None, :])]
    rng2 = np.random.default_rng(2)
    flip = rng2.random(clean.shape, dtype=np.float32) < args.error
    noisy = np.where(flip, (clean + rng2.integers(1, 4, clean.shape, dtype=np.uint8)) % 4, clean).astype(np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    n, m = args.reads, args.length
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(m)
    u32p = ctypes.POINTER(ctypes.c_uint32)

    def index_of(letters):
        """letters: (reads, length) uint8 ASCII"""
        buf = letters.tobytes()
        d = api.DeBWT(k=32)
        t0 = time.perf_counter()
        d.load_ascii([buf[i * m:(i + 1) * m] for i in range(n)])
        d.build()
        fm = d.fm_index(sa_sample=32)
        d.close()
        return fm, buf, time.perf_counter() - t0

    def emit(row):
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as out:
            out.write(json.dumps(row) + "\n")

    def correct(fm, buf, k, flags):
        out = ctypes.create_string_buffer(len(buf))
        info = np.zeros(n, dtype=api._CORRECT_DTYPE)
        o = _lib.DebwtFmCorrectOpts(k=k, min_count=3, max_rounds=4, flags=flags)
        rc = L.debwt_fm_correct(fm._h, buf, api._p64(offs), n, ctypes.byref(o), out, info.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmCorrectInfo)))
        assert rc == 0, fm._L.debwt_fm_last_error(fm._h)
        return np.frombuffer(out.raw, dtype=np.uint8).reshape(n, m), info, fm.correct_stats()

    def overlaps(fm, buf):
        hoff = np.zeros(n + 1, dtype=np.uint64)
        res = fm.overlaps([buf[i * m:(i + 1) * m] for i in range(0, n, max(n // 1000, 1))], min_overlap=args.min_overlap)   # record table
        del res
        rc = L.debwt_fm_overlaps(fm._h, buf, api._p64(offs), n, args.min_overlap, 0, api._p64(hoff), None, 0)
        assert rc in (0, -5)
        total = int(hoff[n])
        hits = np.zeros(max(total, 1), dtype=api._OVERLAP_DTYPE)
        t0 = time.perf_counter()
        rc = L.debwt_fm_overlaps(fm._h, buf, api._p64(offs), n, args.min_overlap, 0, api._p64(hoff),
                                 hits.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmOverlap)), total)
        assert rc == 0
        return total, (time.perf_counter() - t0) * 1e3, fm.overlaps_stats()["ms_kernel"]

    head = {"reads": n, "length": m, "coverage": args.coverage, "genome": G, "error": args.error,
            "substituted_bases": int(flip.sum())}
    noisy_l = acgt[noisy]
    fm, buf, build_s = index_of(noisy_l)
    head["n"] = fm.n
    head["index_build_s"] = round(build_s, 2)

    if args.part == "profile":
        for k in args.k:
            nk = m - k + 1
            total = n * nk
            coff = np.zeros(n + 1, dtype=np.uint64)
            counts = np.zeros(total, dtype=np.uint32)
            flat = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(noisy_l, k, axis=1)).tobytes()   # the exploded list
            foff = np.arange(total + 1, dtype=np.uint64) * np.uint64(k)
            ranges = np.zeros((total, 2), dtype=np.uint64)
            yard, rows = [], []
            for q in (0, 8, 10, 12):
                os.environ["DEBWT_FM_KMER_TABLE_Q"] = str(q)
                rc = L.debwt_fm_kmer_counts(fm._h, buf, api._p64(offs), n, k, 0, api._p64(coff), counts.ctypes.data_as(u32p), total)
                assert rc == 0, fm._L.debwt_fm_last_error(fm._h)
                first = fm.kmer_stats()
                kern, lib = [], []
                for _ in range(args.reps):
                    rc = L.debwt_fm_kmer_counts(fm._h, buf, api._p64(offs), n, k, 0, api._p64(coff), counts.ctypes.data_as(u32p), total)
                    assert rc == 0
                    st = fm.kmer_stats()
                    assert st["ms_table"] == 0
                    kern.append(st["ms_kernel"]); lib.append(st["ms_wall"])
                t0 = time.perf_counter()
                rc = L.debwt_fm_count(fm._h, flat, api._p64(foff), total, api._p64(ranges))
                assert rc == 0
                yard.append((time.perf_counter() - t0) * 1e3)
                assert np.array_equal(counts.astype(np.uint64), ranges[:, 1] - ranges[:, 0])
                rows.append({"part": "profile", "k": k, "q": q, "reps": args.reps, "ms_kernel": spread(kern), "ms_library": spread(lib),
                             "ms_table": round(first["ms_table"], 2), "table_MB": round(16 * 4 ** q / 1e6, 1) if q else 0,
                             "steps": st["steps"], "steps_per_kmer": round(st["steps"] / total, 2),
                             "lines_per_kmer": round(st["line_reads"] / total, 2), "table_starts": st["table_starts"],
                             "busy": round(st["steps"] / max(st["wave_steps"], 1), 3), "batches": st["batches"],
                             "scratch_MB": round(st["scratch_bytes"] / 1e6, 1), "weak_below_3": int((counts < 3).sum())})
            emit({**head, "part": "profile", "k": k, "kmers": total, "yardstick_ms_library": spread(yard),
                  "yardstick_calls": len(yard), "yardstick_bytes": len(flat), "profile_bytes": len(buf), "rows": rows})
            del flat, foff, ranges, counts
    elif args.part == "correct":
        before = int((noisy != clean).sum())
        for name, flags in (("both", 1), ("forward", 0)):
            correct(fm, buf, args.correct_k, flags)                # untimed: the table and the scratch
            fixed, info, st = correct(fm, buf, args.correct_k, flags)
            after = int((fixed != acgt[clean]).sum())
            r = int(st["rounds"])
            emit({**head, "part": "correct", "k": args.correct_k, "min_count": 3, "max_rounds": 4, "strands": name,
                  "ms_library": round(st["ms_wall"], 2), "ms_kernel": round(st["ms_kernel"], 2),
                  "ms_round": [round(x, 2) for x in st["ms_round"][:r]], "reads_fixed_in_round": st["active"][:r],
                  "rounds": r, "trials": st["trials"], "fixes": st["fixes"], "kmers_counted": st["kmers"], "steps": st["steps"],
                  "busy": round(st["steps"] / max(st["wave_steps"], 1), 3), "table_q": st["table_q"], "batches": st["batches"],
                  "scratch_MB": round(st["scratch_bytes"] / 1e6, 1),
                  "reads_clean": st["reads_clean"], "reads_fixed": st["reads_fixed"], "reads_weak": st["reads_weak"],
                  "reads_short": st["reads_short"], "wrong_bases_before": before, "wrong_bases_after": after,
                  "reads_with_errors_before": int((noisy != clean).any(axis=1).sum()),
                  "reads_with_errors_after": int((fixed != acgt[clean]).any(axis=1).sum())})
    else:
        row = {**head, "part": "overlaps", "min_overlap": args.min_overlap, "k": args.correct_k}
        total, ms, msk = overlaps(fm, buf)
        row["uncorrected"] = {"hits": total, "ms_library": round(ms, 2), "ms_kernel": round(msk, 2)}
        correct(fm, buf, args.correct_k, 1)                        # untimed: the table and the scratch
        t0 = time.perf_counter()
        fixed, info, st = correct(fm, buf, args.correct_k, 1)
        t_correct = time.perf_counter() - t0
        fm.close()
        fm2, buf2, t_build = index_of(fixed)
        total2, ms2, msk2 = overlaps(fm2, buf2)
        fm2.close()
        row["corrected"] = {"hits": total2, "ms_library": round(ms2, 2), "ms_kernel": round(msk2, 2),
                            "wrong_bases_after": int((fixed != acgt[clean]).sum()), "correct_s": round(t_correct, 3),
                            "correct_ms_library": round(st["ms_wall"], 2), "rebuild_s": round(t_build, 2),
                            "correct_rebuild_overlaps_s": round(t_correct + t_build + ms2 / 1e3, 2)}
        fm3, buf3, _ = index_of(acgt[clean])
        total3, ms3, msk3 = overlaps(fm3, buf3)
        fm3.close()
        row["error_free"] = {"hits": total3, "ms_library": round(ms3, 2), "ms_kernel": round(msk3, 2)}
        row["corrected_over_error_free"] = round(total2 / max(total3, 1), 4)
        emit(row)
        return
    fm.close()


if __name__ == "__main__":
    main()
