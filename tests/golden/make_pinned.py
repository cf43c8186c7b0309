#!/usr/bin/env python3
"""Store the reference's outputs for the collections of tests/test_oracle_pinned.py under tests/golden/.

Runs the reference's own stage functions (oracle/_ref/ref_driver, built by `make -C oracle ref` where the reference's
sources lie) with `-t 1` on the four formula-defined collections the test pins the oracle with, and writes
pinned_s<seed>.k<k>.{bwt,hash,dollar} (OUT / OUT.# / OUT.$ bytes) and pinned.json (sizes and the sha256 of every
output, kmerInfo included: its ~300 KB per case are kept as a digest only).

    python tests/golden/make_pinned.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O  # noqa: E402
import test_oracle_pinned as P  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    driver = O.build_ref()
    if not driver:
        sys.exit("needs oracle/_ref/ref_driver (make -C oracle ref, with the reference's sources present)")
    cases = []
    for seed, k in P.CASES:
        recs = P.records(seed)
        w, h, d, ki = P._run_ref(driver, recs, k)
        stem = os.path.join(HERE, P.stem(seed, k))
        w.tofile(stem + ".bwt")
        h.tofile(stem + ".hash")
        np.array([d], dtype=np.uint64).tofile(stem + ".dollar")
        cases.append({"seed": seed, "k": k, "n": int(sum(len(r) for r in recs) + len(recs)), "records": len(recs),
                      "distinct_kmers": int(len(ki)),
                      "sha256": {"bwt": sha(w), "hash": sha(h), "dollar": sha(np.array([d], dtype=np.uint64)),
                                 "kmerInfo": sha(ki)}})
        print(f"seed {seed} k {k}: {len(w)} words, {len(h)} '#' rows, '$' row {d}, {len(ki)} k-mers")
    with open(os.path.join(HERE, "pinned.json"), "w") as f:
        json.dump(cases, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
