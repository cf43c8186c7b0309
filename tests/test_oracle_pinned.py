"""Pins the oracle against the reference's own stage functions (oracle/_ref/ref_driver, compiled by oracle/Makefile
from the reference's sources).  Their outputs for the four collections below are committed (tests/golden/pinned.json
and pinned_*.{bwt,hash,dollar}, written by tests/golden/make_pinned.py), so the pin holds wherever the suite runs;
where ref_driver was built, the collections also go through it live and must give the stored bytes."""
import hashlib
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN

CASES = [(1, 32), (2, 16), (3, 12), (4, 27)]


def records(seed):
    from debwt_amd import synth
    return synth.pan_genome(15000 + 1000 * seed, 2 + seed, seed=0xABC0 + seed)


def stem(seed, k):
    return f"pinned_s{seed}.k{k}"


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _run_ref(driver, recs, k, threads=1):
    from debwt_amd import fasta
    d = tempfile.mkdtemp(prefix="pin_")
    try:
        fa, out = os.path.join(d, "in.fa"), os.path.join(d, "OUT")
        fasta.write_fasta(fa, recs)
        p = subprocess.run([driver, d, fa, out, str(k), str(threads)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-800:]
        return (np.fromfile(out, dtype=np.uint64), np.fromfile(out + ".#", dtype=np.uint64),
                int(np.fromfile(out + ".$", dtype=np.uint64)[0]),
                np.fromfile(out + ".kmerInfo", dtype=np.uint64).reshape(-1, 2))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _stored(seed, k):
    entry = {(e["seed"], e["k"]): e for e in json.load(open(os.path.join(GOLDEN, "pinned.json")))}[(seed, k)]
    s = os.path.join(GOLDEN, stem(seed, k))
    w, h = np.fromfile(s + ".bwt", dtype=np.uint64), np.fromfile(s + ".hash", dtype=np.uint64)
    d = np.fromfile(s + ".dollar", dtype=np.uint64)
    assert _sha(w) == entry["sha256"]["bwt"] and _sha(h) == entry["sha256"]["hash"] and _sha(d) == entry["sha256"]["dollar"]
    return w, h, int(d[0]), entry


@pytest.mark.parametrize("seed,k", CASES)
def test_oracle_equals_live_reference(oracle, seed, k):
    recs = records(seed)
    w, h, d, entry = _stored(seed, k)
    driver = oracle.build_ref()
    if driver:                                       # the reference itself is at hand: it still writes the stored bytes
        lw, lh, ld, lki = _run_ref(driver, recs, k)
        assert np.array_equal(lw, w) and np.array_equal(lh, h) and ld == d
        assert _sha(lki) == entry["sha256"]["kmerInfo"]
    sym = oracle.sym_from_codes(recs)
    assert len(sym) == entry["n"]
    ow, oh, od, _ = oracle.build_bwt(sym, k)
    assert np.array_equal(w, ow) and np.array_equal(h, oh) and d == od
    km, ct = oracle.kmer_count(sym, k)
    assert len(km) == entry["distinct_kmers"] and _sha(np.stack([km, ct], axis=1)) == entry["sha256"]["kmerInfo"]
