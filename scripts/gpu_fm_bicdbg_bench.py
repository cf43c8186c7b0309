"""The compacted de Bruijn graph over both strands on one GPU (debwt_fm_cdbg_both), written to a profile.

    python scripts/gpu_fm_bicdbg_bench.py --out profiles/r29_fm_cdbg_both.txt

The reads of scripts/gpu_fm_esa_bench.py (same function, same seeds) with every second read reverse-complemented, in a child
process of its own under --step-timeout seconds.  Per k of --ks:

part "esa"      debwt_fm_esa_build with max_lcp = k + 1, sa and da, on the index of the reads (ms_wall, bytes).
part "forward"  debwt_fm_cdbg on that index: --reps sizing calls and --reps writing calls, each after one untimed.
part "both"     debwt_fm_cdbg_both on that index, the same way: ms per phase (nodes, mates, links, rank, write) and ms_wall,
                scratch_bytes, the counting fields, mated share, hairpins, mate_steps, edge_keys, N50.
part "route"    the way without the feature, once: BWT and index of the doubled reads (every read and its reverse
                complement), debwt_fm_esa_build and debwt_fm_cdbg on it, and a fold on the host (each unitig string under
                the lower of itself and its reverse complement).  The folded unitigs (string, kmer_count) are compared with
                those of part "both": the row counts the ones that differ, and asserts that none does where hairpins = 0.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from gpu_fm_cdbg_bench import emit, n50  # noqa: E402
from gpu_fm_esa_bench import read_set, spread  # noqa: E402

F_PHASES = ("ms_nodes", "ms_links", "ms_rank", "ms_write", "ms_wall")
B_PHASES = ("ms_nodes", "ms_mates", "ms_links", "ms_rank", "ms_write", "ms_wall")
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return s.translate(COMP)[::-1]


def canonical(G, k):
    """{the lower of a unitig's string and its reverse complement: kmer_count}"""
    seq = G.seq.tobytes()
    out = {}
    for off, m, kc in zip(G.unitigs["seq_offset"].tolist(), (G.unitigs["nodes"].astype(np.int64) + k - 1).tolist(),
                          G.unitigs["kmer_count"].tolist()):
        s = seq[off:off + m]
        out[min(s, rc(s))] = kc
    return out


def index_of(api, recs):
    d = api.DeBWT(k=32)
    t0 = time.perf_counter()
    d.load_ascii(recs)
    d.build()
    fm = d.fm_index(sa_sample=32)
    d.close()
    return fm, round(time.perf_counter() - t0, 2)


def timed(call, stats, reps):
    call()
    rows = []
    for _ in range(reps):
        G = call()
        rows.append(stats())
    return G, rows


def run(args):
    from debwt_amd import _lib, api
    recs, head = read_set(args)
    recs = [rc(r) if i & 1 else r for i, r in enumerate(recs)]
    fm, index_s = index_of(api, recs)
    head = {**head, "every_second_read": "reverse-complemented", "n": fm.info()["n"], "nrec": fm.info()["nrec"], "index_s": index_s}
    both = {}
    for k in args.ks:
        fm.esa(max_lcp=k + 1, sa=True, da=True)                         # the text is restored by the first
        e = fm.esa(max_lcp=k + 1, sa=True, da=True)
        es = fm.esa_stats()
        emit(args, {**head, "part": "esa", "k": k, "esa_build_ms": round(es["ms_wall"], 1), "kept_bytes": es["kept_bytes"]})

        def sizing(entry, stats):
            sz = _lib.DebwtFmCdbgSizes()
            rc_ = entry(fm._h, k, 0, None, 0, None, 0, None, 0, ctypes.byref(sz))
            assert rc_ in (0, -5), rc_

        for part, entry, stats, phases, kw in (("forward", fm._L.debwt_fm_cdbg, fm.cdbg_stats, F_PHASES, {}),
                                               ("both", fm._L.debwt_fm_cdbg_both, fm.cdbg_both_stats, B_PHASES, {"strands": "both"})):
            _, rows = timed(lambda: sizing(entry, stats), stats, args.reps)
            G, full = timed(lambda: e.cdbg(k, **kw), stats, args.reps)
            st = full[-1]
            emit(args, {"part": part, "k": k, "reps": args.reps,
                        "sizing": {p: spread([r[p] for r in rows]) for p in phases},
                        "writing": {p: spread([r[p] for r in full]) for p in phases},
                        "N50": n50(G.unitigs["nodes"].astype(np.int64) + k - 1),
                        **({"mated_share": round(st["mated"] / max(st["present"], 1), 4)} if part == "both" else {}),
                        **{c: v for c, v in st.items() if not c.startswith("ms_")}})
            if part == "both":
                both[k] = (canonical(G, k), st["hairpins"])
            del G
    fm.close()
    t0 = time.perf_counter()
    doubled = [x for r in recs for x in (r, rc(r))]
    host_s = round(time.perf_counter() - t0, 2)
    del recs
    fd, index_s = index_of(api, doubled)
    del doubled
    for k in args.ks:
        fd.esa(max_lcp=k + 1, sa=True, da=True)
        e = fd.esa(max_lcp=k + 1, sa=True, da=True)
        es = fd.esa_stats()
        G = e.cdbg(k)
        G = e.cdbg(k)
        st = fd.cdbg_stats()
        t0 = time.perf_counter()
        folded = canonical(G, k)
        fold_ms = round((time.perf_counter() - t0) * 1e3, 1)
        want, hairpins = both[k]
        differ = len(set(folded.items()) ^ set(want.items()))
        assert hairpins or not differ, differ
        emit(args, {"part": "route", "k": k, "what": "the doubled reads: BWT and index, esa build, debwt_fm_cdbg, fold on the host; one run",
                    "doubling_on_host_s": host_s, "index_s": index_s, "n": fd.info()["n"], "esa_build_ms": round(es["ms_wall"], 1),
                    "kept_bytes": es["kept_bytes"], "cdbg_ms_wall": round(st["ms_wall"], 1), "cdbg_scratch_bytes": st["scratch_bytes"],
                    "unitigs_of_D": len(G.unitigs), "fold_ms": fold_ms, "folded_unitigs": len(folded), "unitigs_of_both": len(want),
                    "hairpins": hairpins, "records_that_differ": differ})
        del G
    fd.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--ks", type=int, nargs="+", default=[21, 31])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_cdbg_both.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        run(args)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--out", args.out, "--reads", str(args.reads),
           "--length", str(args.length), "--coverage", str(args.coverage), "--error", str(args.error), "--reps", str(args.reps),
           "--ks", *[str(c) for c in args.ks]]
    rc_ = subprocess.run(cmd, timeout=args.step_timeout).returncode            # a fresh process; a failure ends the script
    if rc_:
        sys.exit(f"exit status {rc_}")


if __name__ == "__main__":
    main()
