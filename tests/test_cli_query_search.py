"""deBWT-query count / locate with --mismatches, --both-strands and --best (debwt_fm_search) against a Python Hamming
scan of the records; without them the output stays that of the plain commands."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(*args):
    return subprocess.run([QUERY, *args], capture_output=True, text=True, timeout=300)


def _revcomp(p):
    return "".join(COMP.get(c, "N") for c in reversed(p.upper()))


def _scan(recs, pat, K, both, best):
    """sorted (record, offset, strand, mismatches) of every window within Hamming distance K"""
    out = []
    for strand, q in ((0, pat.upper()), (1, _revcomp(pat))):
        if strand and not both:
            break
        if not q:
            continue
        for i, r in enumerate(recs):
            for o in range(len(r) - len(q) + 1):
                d = sum(1 for a, b in zip(r[o:o + len(q)], q) if a != b or b not in "ACGT")
                if d <= K:
                    out.append((i, o, strand, d))
    if best and out:
        low = min(x[3] for x in out)
        out = [x for x in out if x[3] == low]
    return sorted(out)


def test_search_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    for v in ("5", "x", "-1"):
        r = _run("count", "-i", str(tmp_path / "o"), "--mismatches", v, "p.fa")
        assert r.returncode == 1 and "--mismatches" in r.stderr
    r = _run("index", "-i", str(tmp_path / "o"), "--mismatches", "1", "x.fa")
    assert r.returncode == 1 and "usage" in r.stderr


@pytest.mark.gpu
def test_search_end_to_end(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    from debwt_amd import fasta
    fa = os.path.join(GOLDEN, "shared_ends_duplicates.fa")
    recs = ["".join("ACGT"[c] for c in r) for r in fasta.read_fasta(fa)[1]]
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, fa], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", fa)
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(3)
    pats = []
    for i in range(24):
        rec = recs[int(rng.integers(0, len(recs)))]
        L = int(rng.integers(6, 30))
        p = int(rng.integers(0, len(rec) - L))
        s = list(rec[p:p + L])
        for _ in range(int(rng.integers(0, 3))):
            s[int(rng.integers(0, L))] = "ACGT"[int(rng.integers(0, 4))]
        s = "".join(s)
        if i % 4 == 0:
            s = _revcomp(s)
        if i % 7 == 0:
            s = s.lower()
        pats.append(s)
    pats += ["ACGTNACGT", ""]
    pf = tmp_path / "p.fa"
    pf.write_text("".join(f">q{i}\n{p}\n" for i, p in enumerate(pats)))
    for K in (1, 2):
        for both in (False, True):
            for best in (False, True):
                opts = ["--mismatches", str(K)] + (["--both-strands"] if both else []) + (["--best"] if best else [])
                want = [_scan(recs, p, K, both, best) for p in pats]
                r = _run("count", "-i", out, *opts, str(pf))
                assert r.returncode == 0, r.stderr
                lines = r.stdout.splitlines()
                assert len(lines) == len(pats)
                for i, (line, w) in enumerate(zip(lines, want)):
                    per = [sum(1 for x in w if x[3] == k) for k in range(K + 1)]
                    assert line == f"q{i}\t{len(w)}\t" + ",".join(map(str, per)), (opts, pats[i])
                r = _run("locate", "-i", out, *opts, str(pf))
                assert r.returncode == 0, r.stderr
                for i, (line, w) in enumerate(zip(r.stdout.splitlines(), want)):
                    hits = ",".join(f"{a}:{b}:{'+-'[s]}:{d}" for a, b, s, d in w)
                    assert line == f"q{i}\t{len(w)}\t{hits}", (opts, pats[i])
                r = _run("locate", "-i", out, "--max-hits", "3", *opts, str(pf))
                assert r.returncode == 0, r.stderr
                for i, (line, w) in enumerate(zip(r.stdout.splitlines(), want)):
                    hits = ",".join(f"{a}:{b}:{'+-'[s]}:{d}" for a, b, s, d in w[:3])
                    assert line == f"q{i}\t{len(w)}\t{hits}", (opts, pats[i])
    # without the new options: the plain commands' output, unchanged
    r0 = _run("count", "-i", out, str(pf))
    assert r0.returncode == 0 and all(len(x.split("\t")) == 2 for x in r0.stdout.splitlines())
    r1 = _run("locate", "-i", out, "--max-hits", "2", str(pf))
    assert r1.returncode == 0 and all(len(x.split("\t")) == 3 and x.count(":") <= 2 for x in r1.stdout.splitlines())
    r = _run("count", "-i", out, "--mismatches", "0", str(pf))
    assert r.returncode == 0
    for a, b in zip(r0.stdout.splitlines(), r.stdout.splitlines()):
        assert b == a + "\t" + a.split("\t")[1]
