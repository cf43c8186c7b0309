"""deBWT-query overlaps --max-mismatches / --max-error-permille (debwt_fm_overlaps_mm): option errors without a GPU; on the
GPU, deBWT, index and overlaps on a FASTA of the mutated read set, queried with itself, line by line against the
reference of overlap_mm_ref.py with the sixth column, and without the new option the five columns as before."""
import os
import subprocess

import pytest

from conftest import ROOT
from overlap_mm_ref import brute, mutated_reads
from overlap_ref import CONTAINS, WHOLE, Ref, longest_of, revcomp

CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")
NAMES = {0: ".", CONTAINS: "C", WHOLE: "W", CONTAINS | WHOLE: "CW"}


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(*args):
    return subprocess.run([QUERY, *args], capture_output=True, text=True, timeout=300)


def test_overlaps_mm_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    out = str(tmp_path / "o")
    for v in ("5", "x", "-1", ""):
        r = _run("overlaps", "-i", out, "--max-mismatches", v, "p.fa")
        assert r.returncode == 1 and "--max-mismatches" in r.stderr and "usage" not in r.stderr
    for v in ("1001", "x", "-1"):
        r = _run("overlaps", "-i", out, "--max-mismatches", "1", "--max-error-permille", v, "p.fa")
        assert r.returncode == 1 and "--max-error-permille" in r.stderr and "usage" not in r.stderr
    r = _run("overlaps", "-i", out, "--max-error-permille", "50", "p.fa")
    assert r.returncode == 1 and "--max-error-permille" in r.stderr and "usage" in r.stderr
    for cmd in ("count", "mems"):
        for opt in (["--max-mismatches", "1"], ["--max-error-permille", "50"]):
            r = _run(cmd, "-i", out, *opt, "p.fa")
            assert r.returncode == 1 and "usage" in r.stderr


@pytest.mark.gpu
def test_overlaps_mm_end_to_end(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    strs, _ = mutated_reads()
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(strs)))
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, str(fa)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", str(fa))
    assert r.returncode == 0, r.stderr
    for permille, both, longest, no_self in ((0, False, False, False), (50, True, True, True), (50, False, False, True),
                                             (0, True, False, False)):
        opts = ["--max-mismatches", "2"] + (["--max-error-permille", str(permille)] if permille else []) + \
               (["--both-strands"] if both else []) + (["--longest"] if longest else []) + (["--no-self"] if no_self else [])
        r = _run("overlaps", "-i", out, *opts, str(fa))
        assert r.returncode == 0, r.stderr
        want, with_mm = [], 0
        for i, p in enumerate(strs):
            hits = brute(strs, p, 20, 2, permille) + (brute(strs, revcomp(p), 20, 2, permille, strand=1) if both else [])
            if longest:
                hits = longest_of(hits)
            for j, L, strand, fl in hits:
                if no_self and strand == 0 and j == i and L == len(p):
                    continue
                want.append(f"r{i}\t{'+-'[strand]}\t{j}\t{L}\t{NAMES[fl & 3]}\t{fl >> 8}")
                with_mm += fl >> 8 > 0
        lines = r.stdout.splitlines()
        assert len(lines) == len(want), opts
        for got, w in zip(lines, want):
            assert got == w, opts
        assert len(want) > len(strs) and with_mm > 0
    # K = 0 through the new call: the exact overlaps with a sixth column of zeros
    R = Ref(strs, 20)
    want5 = [f"r{i}\t+\t{j}\t{L}\t{NAMES[fl]}" for i, p in enumerate(strs) for j, L, _, fl in R.hits(p)]
    r = _run("overlaps", "-i", out, "--max-mismatches", "0", str(fa))
    assert r.returncode == 0 and r.stdout.splitlines() == [w + "\t0" for w in want5]
    # without the new option: the five columns, byte for byte
    r = _run("overlaps", "-i", out, str(fa))
    assert r.returncode == 0 and r.stdout == "".join(w + "\n" for w in want5)
