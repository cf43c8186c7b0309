"""Extract and text restore on one GPU (debwt_fm_extract, debwt_fm_restore_text): anchors, kernel and wall time and the
share of lanes busy, beside the verifier's walk of the same rows, written to a profile.

    python scripts/gpu_fm_extract_bench.py --workloads pan1x3.1G --out profiles/r16_fm_extract.txt

Per workload: build the BWT, make the index at s = 32 and keep its samples; run debwt_verify_device on the context's own
rows at its default segment count (ms_walk: the same n LF steps over evenly long segments, compared with the text, no
stores); fetch the rows and open a second index from rows and samples alone.  On that index: debwt_fm_restore_text (ms to
build the anchors, ms_kernel, ms_wall, steps / wave_steps), then the restored words compared with the text the build was
loaded with; debwt_fm_extract of --short jobs of 150 bases at random places and of --long jobs of 10^5 bases, one
untimed call of each shape first, then --reps timed ones (median, smallest, largest).  For context, the host route the
restore replaces: debwt_fm_attach_text of the packed words from host memory on a third index (the packing of a FASTA
file, debwt_pack_fasta, is not part of it: there is no file here; its rate is in the ingest profiles)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JOB = np.dtype([("record", np.uint32), ("reserved", np.uint32), ("offset", np.uint64), ("length", np.uint64)])


def spread(v):
    return [round(float(np.median(v)), 2), round(float(min(v)), 2), round(float(max(v)), 2)]


def extract(fm, jobs, buf):
    """one debwt_fm_extract call over a numpy job array into buf; returns the bases written"""
    from debwt_amd import _lib
    offs = np.zeros(len(jobs) + 1, dtype=np.uint64)
    rc = fm._L.debwt_fm_extract(fm._h, jobs.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmExtractJob)), len(jobs),
                                offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                buf.ctypes.data_as(ctypes.c_char_p), len(buf))
    fm._chk(rc)
    return offs


def run(name, args, out):
    from debwt_amd import api
    from debwt_amd import synth_native as SN
    syn = SN.Synth.named(name)
    n, nrec = syn.n, syn.nrec
    sep = np.asarray(syn.sep(), dtype=np.uint64)
    text = SN.PinnedArray(syn.nwords)
    syn.words_into(text.ptr)
    words = text.a
    d = api.DeBWT(k=32)
    d.load_packed(words, n, sep)
    d.build()
    ver = d.verify_device()
    assert ver["inverse_bwt_ok"]
    fm0 = d.fm_index(sa_sample=args.sa)
    sa = fm0.samples()
    fm0.close()
    rows = d.fetch()
    d.close()
    res = {"workload": name, "n": n, "nrec": nrec, "sa_sample": args.sa,
           "verify": {k: ver["inverse_bwt"][k] for k in ("segments", "steps", "ms_walk", "ms_search")}}
    # the host route: the packed text uploaded and checked
    fm = api.FMIndex.open(rows[0], n, rows[1], rows[2], sa, sa_sample=args.sa)
    t0 = time.perf_counter()
    fm.attach_text(words=words, sep=sep)
    res["attach_text_from_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    fm.close()
    # restore
    fm = api.FMIndex.open(rows[0], n, rows[1], rows[2], sa, sa_sample=args.sa)
    before = fm.info()["device_bytes"]
    t0 = time.perf_counter()
    fm.restore_text()
    wall = (time.perf_counter() - t0) * 1e3
    st = fm.extract_stats()
    got, gsep = fm.text()
    body = (n + 63) >> 5
    same = bool(np.array_equal(got[:body], words[:body]) and not got[body:].any() and np.array_equal(gsep, sep))
    res["restore"] = {"ms_anchors": round(st["ms_anchors"], 2), "ms_kernel": round(st["ms_kernel"], 2),
                      "ms_library": round(st["ms_wall"], 2), "wall_ms": round(wall, 2), "segments": st["segments"],
                      "steps": st["steps"], "busy": round(st["steps"] / max(st["wave_steps"], 1), 3),
                      "anchor_bytes": st["anchor_bytes"], "device_GB_before": round(before / 1e9, 2),
                      "device_GB_after": round(fm.info()["device_bytes"] / 1e9, 2), "equals_loaded_text": same,
                      "kernel_over_verify_walk": round(st["ms_kernel"] / max(ver["inverse_bwt"]["ms_walk"], 1e-9), 2)}
    print(json.dumps(res), flush=True)
    assert same
    # extract
    rng = np.random.default_rng(1)
    starts = fm.record_starts().astype(np.int64)
    lens = np.append(starts[1:], n).astype(np.int64) - 1 - starts
    res["extract"] = []
    for count, length in ((args.short, 150), (args.long, 100_000)):
        ok = np.nonzero(lens >= length)[0]
        rec = ok[rng.integers(0, len(ok), count)]
        jobs = np.zeros(count, dtype=JOB)
        jobs["record"] = rec
        jobs["offset"] = (rng.random(count) * (lens[rec] - length + 1)).astype(np.uint64)
        jobs["length"] = length
        buf = np.zeros(count * length, dtype=np.uint8)
        extract(fm, jobs, buf)
        kern, lib, wl = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            offs = extract(fm, jobs, buf)
            wl.append((time.perf_counter() - t0) * 1e3)
            st = fm.extract_stats()
            kern.append(st["ms_kernel"])
            lib.append(st["ms_wall"])
        # spot check against the loaded text
        for j in rng.integers(0, count, 50):
            a = int(starts[jobs["record"][j]]) + int(jobs["offset"][j])
            idx = np.arange(a, a + length)
            codes = ((words[idx >> 5] >> (2 * (31 - (idx & 31))).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)
            assert buf[int(offs[j]):int(offs[j + 1])].tobytes() == np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes()
        bases = int(offs[-1])
        row = {"jobs": count, "length": length, "bases": bases, "reps": args.reps, "ms_kernel": spread(kern),
               "ms_library": spread(lib), "wall_ms": spread(wl), "bases_per_s_kernel": round(bases / np.median(kern) * 1e3),
               "bases_per_s_library": round(bases / np.median(lib) * 1e3), "segments": st["segments"], "steps": st["steps"],
               "steps_per_base": round(st["steps"] / bases, 2), "busy": round(st["steps"] / max(st["wave_steps"], 1), 3),
               "batches": st["batches"], "launches": st["launches"], "anchor_bytes": st["anchor_bytes"]}
        res["extract"].append(row)
        print(json.dumps(row), flush=True)
    fm.close()
    text.free()
    syn.close()
    out.write(json.dumps(res) + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pan1x3.1G")
    ap.add_argument("--sa", type=int, default=32)
    ap.add_argument("--short", type=int, default=1_000_000)
    ap.add_argument("--long", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "fm_extract.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as out:
        for name in args.workloads.split(","):
            run(name, args, out)


if __name__ == "__main__":
    main()
