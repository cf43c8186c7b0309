"""Suffix array, LCP array and record array on one GPU (debwt_fm_esa_build), written to a profile.

    python scripts/gpu_fm_esa_bench.py --out profiles/r25_fm_esa.txt

Two workloads, each in a child process of its own under --step-timeout seconds (the first failure ends the script):

reads    the read set of scripts/gpu_fm_kmer_bench.py (same seeds: `reads` reads of `length` bases at uniform positions of
         a random genome of reads x length / coverage bases, every base substituted with probability --error), indexed at
         s = 32 against itself.
genome   one record of --genome random bases in which --repeats stretches of --repeat-length bases are copied to another
         place with one base in 1000 changed, so that the LCP array has long values and the carry has work; s = 32.

Per workload: the text is restored once (untimed for the builds that follow), then --reps builds each of lcp alone and of
lcp + sa + da.  Per phase (walk, scatter, PLCP, rows with the reductions) the ms from events; symbols_compared / n; the
busy share of the walk (steps / wave_steps) and of the PLCP kernel (word steps / plcp_wave_steps); bytes while building
and kept; the summary.  Then the chunk lengths of --chunks (the default is 256): ms of the PLCP phase and symbols / n.
Beside it, in the same process, the route without the feature: debwt_fm_locate over the one range [0, n), which is the
whole suffix array through the samples, checked equal to the kept array.  Every list is [median, smallest, largest]."""
import argparse
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


def read_set(args):
    rng = np.random.default_rng(1)
    n, m = args.reads, args.length
    G = int(n * m / args.coverage)
    genome = rng.integers(0, 4, G).astype(np.uint8)              # codes; the same draws as gpu_fm_kmer_bench.py
    starts = rng.integers(0, G - m + 1, n)
    clean = genome[(starts[:, None] + np.arange(m)[None, :])]
    rng2 = np.random.default_rng(2)
    flip = rng2.random(clean.shape, dtype=np.float32) < args.error
    noisy = np.where(flip, (clean + rng2.integers(1, 4, clean.shape, dtype=np.uint8)) % 4, clean).astype(np.uint8)
    buf = np.frombuffer(b"ACGT", dtype=np.uint8)[noisy].tobytes()
    return [buf[i * m:(i + 1) * m] for i in range(n)], {"reads": n, "length": m, "coverage": args.coverage, "error": args.error}


def genome(args):
    rng = np.random.default_rng(3)
    G, L = args.genome, args.repeat_length
    g = rng.integers(0, 4, G, dtype=np.uint8)
    for _ in range(args.repeats):
        a, b = (int(x) for x in rng.integers(0, G - L, 2))
        piece = g[a:a + L].copy()
        hit = rng.random(L) < 0.001
        piece[hit] = (piece[hit] + 1) % 4
        g[b:b + L] = piece
    return [np.frombuffer(b"ACGT", dtype=np.uint8)[g].tobytes()], {"genome": G, "repeats": args.repeats, "repeat_length": L}


def run(which, args):
    from debwt_amd import api
    recs, head = read_set(args) if which == "reads" else genome(args)
    d = api.DeBWT(k=32)
    t0 = time.perf_counter()
    d.load_ascii(recs)
    del recs
    d.build()
    fm = d.fm_index(sa_sample=32)
    d.close()
    n = fm.info()["n"]
    head = {"workload": which, **head, "n": n, "nrec": fm.info()["nrec"], "sa_sample": 32,
            "index_build_s": round(time.perf_counter() - t0, 2)}
    t0 = time.perf_counter()
    fm.restore_text()
    head["restore_text_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    os.environ.pop("DEBWT_FM_ESA_CHUNK", None)

    def build(**kw):
        e = fm.esa(**kw)
        return e, fm.esa_stats()

    for name, kw in (("lcp", {}), ("lcp+sa+da", {"sa": True, "da": True})):
        build(**kw)
        rows = []
        for _ in range(args.reps):
            e, st = build(**kw)
            rows.append(st)
        sm = e.summary()
        emit(args, {**head, "part": "build", "arrays": name, "reps": args.reps,
                    **{k: spread([r[k] for r in rows]) for k in ("ms_walk", "ms_scatter", "ms_plcp", "ms_rows", "ms_wall")},
                    "symbols_per_position": round(st["symbols_compared"] / n, 3),
                    "walk_items": st["walk_items"], "walk_busy": round(st["walk_steps"] / max(st["walk_wave_steps"], 1), 3),
                    "plcp_busy": round(st["symbols_compared"] / 32 / max(st["plcp_wave_steps"], 1), 3),
                    "chunks": st["chunks"], "chunk_len": st["chunk_len"], "build_MB": round(st["build_bytes"] / 1e6, 1),
                    "kept_MB": round(st["kept_bytes"] / 1e6, 1), "max": sm["max"], "max_row": sm["max_row"],
                    "mean": round(sm["sum"] / n, 3), "distinct_k": {str(k): int(e.profile(32)[k - 1]) for k in (12, 21, 32)}})
    t0 = time.perf_counter()
    sa = e.sa()
    fetch = (time.perf_counter() - t0) * 1e3
    lcp = e.lcp()
    rows = []
    for chunk in args.chunks:
        os.environ["DEBWT_FM_ESA_CHUNK"] = str(chunk)
        build()
        ms = []
        for _ in range(3):
            e2, st = build()
            ms.append(st["ms_plcp"])
        assert np.array_equal(e2.lcp(), lcp)
        rows.append({"chunk": chunk, "chunks": st["chunks"], "ms_plcp": spread(ms),
                     "symbols_per_position": round(st["symbols_compared"] / n, 3),
                     "plcp_busy": round(st["symbols_compared"] / 32 / max(st["plcp_wave_steps"], 1), 3)})
    os.environ.pop("DEBWT_FM_ESA_CHUNK", None)
    emit(args, {"part": "chunks", "workload": which, "rows": rows})
    # the route without the feature: locate every row through the samples
    rng_ = np.array([[0, n]], dtype=np.uint64)
    offs = np.zeros(2, dtype=np.uint64)
    pos = np.empty(n, dtype=np.uint64)
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        rc = fm._L.debwt_fm_locate(fm._h, api._p64(rng_), 1, 0, api._p64(offs), api._p64(pos), n)
        assert rc == 0
        ms.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(pos, sa)
    emit(args, {"part": "route", "workload": which, "what": "debwt_fm_locate over [0, n), host time with its copies to the host",
                "ms": spread(ms), "equal_to_kept_sa": True, "fetch_kept_sa_ms": round(fetch, 1)})
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
    ap.add_argument("--genome", type=int, default=1 << 28)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--repeat-length", type=int, default=20000)
    ap.add_argument("--chunks", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", nargs="+", default=["reads", "genome"])
    ap.add_argument("--step-timeout", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_esa.txt"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        run(args.child, args)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for which in args.workloads:                                  # a fresh process per workload; a failure ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--out", args.out, "--reads", str(args.reads),
               "--length", str(args.length), "--coverage", str(args.coverage), "--error", str(args.error),
               "--genome", str(args.genome), "--repeats", str(args.repeats), "--repeat-length", str(args.repeat_length),
               "--reps", str(args.reps), "--chunks", *[str(c) for c in args.chunks]]
        rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        if rc:
            sys.exit(f"{which}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
