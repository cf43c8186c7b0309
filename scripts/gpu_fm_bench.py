"""FM-index on one GPU (debwt_fm_*): sample build, count and locate rates on distribution P, written to a profile.

    python scripts/gpu_fm_bench.py --workloads pan1x3.1G,pan10x3G --out profiles/r07_fm_index.txt

Per workload: build the BWT (debwt_build), make the index at s = 32 (rank lines + the verifier's walk with the sample
stores), then count 10^6 patterns of 32 b and of 100 b drawn from the text (10 % with one base changed) and locate the
occurrences of 10^5 of the 32 b patterns.  Times are host wall times of the library calls (pattern upload and result
download included); line rates count 128-byte rank lines: count <= 2 per pattern symbol (lo and hi), locate ~ s per
occurrence (the expected walk to a sampled row)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def draw(words, sep, n, L, count, rng, mutate=0.1):
    """count patterns of L bases at random text positions that cross no separator, 10 % with one base changed"""
    pos = rng.integers(0, n - L, size=count * 2, dtype=np.int64)
    ok = np.searchsorted(sep, pos) == np.searchsorted(sep, pos + L)
    pos = pos[ok][:count]
    idx = pos[:, None] + np.arange(L)[None, :]
    codes = ((words[idx >> 5] >> (2 * (31 - (idx & 31))).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)
    m = rng.random(len(codes)) < mutate
    codes[m, rng.integers(0, L, size=int(m.sum()))] = rng.integers(0, 4, size=int(m.sum())).astype(np.uint8)
    return [bytes(r) for r in np.frombuffer(b"ACGT", dtype=np.uint8)[codes]]


def run(name, args, out):
    from debwt_amd import api
    from debwt_amd import synth_native as SN
    t0 = time.perf_counter()
    syn = SN.Synth.named(name)
    n, nrec = syn.n, syn.nrec
    sep = np.asarray(syn.sep(), dtype=np.int64)
    text = SN.PinnedArray(syn.nwords)
    syn.words_into(text.ptr)
    words = text.a
    t_gen = time.perf_counter() - t0
    d = api.DeBWT(k=32)
    d.load_packed(words, n, sep.astype(np.uint64))
    t0 = time.perf_counter()
    d.build()
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    fm = d.fm_index(sa_sample=args.sa)
    t_index = time.perf_counter() - t0
    info = fm.info()
    d.close()                                                  # the index outlives the context: its HBM goes back
    rng = np.random.default_rng(1)
    res = {"workload": name, "n": n, "nrec": nrec, "sa_sample": args.sa, "generate_s": round(t_gen, 2),
           "build_s": round(t_build, 2), "index_wall_s": round(t_index, 3), "rank_ms": round(info["ms_rank"], 1),
           "samples_ms": round(info["ms_samples"], 1), "index_device_GB": round(info["device_bytes"] / 1e9, 2)}
    for L in (32, 100):
        pats = draw(words, sep, n, L, args.patterns, rng)
        fm.count(pats[:1000])                                  # scratch allocated outside the timing
        t0 = time.perf_counter()
        r = fm.ranges(pats)
        dt = time.perf_counter() - t0
        c = r[:, 1] - r[:, 0]
        lines = 2 * L * len(pats)
        res[f"count_{L}b"] = {"patterns": len(pats), "s": round(dt, 4), "patterns_per_s": round(len(pats) / dt),
                              "found": int((c > 0).sum()), "lines_le": lines,
                              "line_GBps_le": round(lines * 128 / dt / 1e9, 1)}
        if L == 32:
            sub = pats[:args.locate]
            fm.locate(sub[:100])
            t0 = time.perf_counter()
            loc = fm.locate(sub, max_per_pattern=args.max_hits)
            dt = time.perf_counter() - t0
            occ = sum(len(x) for x in loc)
            res["locate_32b"] = {"patterns": len(sub), "occurrences": occ, "s": round(dt, 4),
                                 "occurrences_per_s": round(occ / dt), "lines_est": occ * args.sa,
                                 "line_GBps_est": round(occ * args.sa * 128 / dt / 1e9, 1)}
    fm.close()
    text.free()
    syn.close()
    out.write(json.dumps(res) + "\n")
    out.flush()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pan1x3.1G,pan10x3G")
    ap.add_argument("--sa", type=int, default=32)
    ap.add_argument("--patterns", type=int, default=1_000_000)
    ap.add_argument("--locate", type=int, default=100_000)
    ap.add_argument("--max-hits", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_index.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as out:
        for name in args.workloads.split(","):
            run(name, args, out)


if __name__ == "__main__":
    main()
