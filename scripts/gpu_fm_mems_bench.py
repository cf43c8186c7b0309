"""Maximal exact matches on one GPU (debwt_fm_mems): kernel and wall time, MEMs, rank steps and lines per read and the
share of lanes busy (divergence), written to a profile.

    python scripts/gpu_fm_mems_bench.py --workloads pan1x3.1G --out profiles/r09_fm_mems.txt

Per workload: build the BWT, make the index at s = 32, draw 10^6 reads of 150 b: from the text with 0..4 random
substitutions (gpu_fm_bench.draw, then the changes), a share of random reads and a share of chimeras of two distant
pieces of 75 b.  MEMs of at least --min-len bases (default 19) on the forward strand and on both.  ms_kernel sums the
k_fm_mems launches by events; wall_s is the host time of FMIndex.mems (upload, launches, compaction, download).
busy = rank steps / wave steps: the share of a wave's lanes that take a step, on average, while the wave still runs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def substitute(pats, K, rng):
    """each pattern with 0..K random substitutions (uniform number, positions and letters)"""
    out = []
    for p in pats:
        b = bytearray(p)
        for _ in range(int(rng.integers(0, K + 1))):
            b[int(rng.integers(0, len(b)))] = b"ACGT"[int(rng.integers(0, 4))]
        out.append(bytes(b))
    return out


def reads(words, sep, n, count, length, random_share, chimera_share, rng):
    from gpu_fm_bench import draw
    nrand, nchim = int(count * random_share), int(count * chimera_share)
    nsub = count - nrand - nchim
    out = substitute(draw(words, sep, n, length, nsub, rng, mutate=0.0), 4, rng)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out += [acgt[rng.integers(0, 4, length)].tobytes() for _ in range(nrand)]
    half = length // 2
    a = draw(words, sep, n, half, nchim, rng, mutate=0.0)
    b = draw(words, sep, n, length - half, nchim, rng, mutate=0.0)
    out += [x + y for x, y in zip(a, b)]                     # two random text positions: distant almost surely
    return [out[i] for i in rng.permutation(len(out))]


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
    d.close()
    rng = np.random.default_rng(1)
    rs = reads(text.a, sep, n, args.reads, args.length, args.random, args.chimeras, rng)
    res = {"workload": name, "n": n, "nrec": nrec, "reads": len(rs), "length": args.length, "min_len": args.min_len,
           "random_share": args.random, "chimera_share": args.chimeras, "runs": []}
    for strands in ("forward", "both"):
        fm.mems(rs[:1000], min_len=args.min_len, strands=strands)      # scratch allocated outside the timing
        t0 = time.perf_counter()
        mr = fm.mems(rs, min_len=args.min_len, strands=strands)
        wall = time.perf_counter() - t0
        st = fm.mems_stats()
        nm = int(mr.offsets[-1])
        row = {"strands": strands, "wall_s": round(wall, 4), "ms_kernel": round(st["ms_kernel"], 2),
               "ms_library": round(st["ms_wall"], 2), "reads_per_s": round(len(rs) / wall),
               "mems": nm, "mems_per_read": round(nm / len(rs), 3),
               "reads_with_mems": int((np.diff(mr.offsets) > 0).sum()),
               "steps_per_read": round(st["steps"] / len(rs), 1), "lines_per_read": round(st["line_reads"] / len(rs), 1),
               "busy": round(st["steps"] / max(st["wave_steps"], 1), 3), "batches": st["batches"],
               "launches": st["launches"], "slot_scratch_GB": round(st["scratch_bytes"] / 1e9, 2)}
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
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--min-len", type=int, default=19)
    ap.add_argument("--random", type=float, default=0.05, help="share of random reads")
    ap.add_argument("--chimeras", type=float, default=0.05, help="share of chimeras of two distant pieces")
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_mems.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as out:
        for name in args.workloads.split(","):
            run(name, args, out)


if __name__ == "__main__":
    main()
