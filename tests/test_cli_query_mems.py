"""deBWT-query mems (debwt_fm_mems): option errors without a GPU; on the GPU, index then mems on a golden FASTA with
--both-strands and --max-hits, line by line against a Python brute force over the records."""
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


def _mems(recs, p, min_len, both):
    """(strand, qbeg, qend, string) per MEM from the definition, ascending by (strand, qbeg)"""
    def occurs(w):
        return any(w in r for r in recs)
    out, m = [], len(p)
    for strand, q in ((0, p.upper()), (1, _revcomp(p))):
        if strand and not both:
            break
        s, se = 0, []
        for e in range(m):
            while s <= e and not occurs(q[s:e + 1]):
                s += 1
            se.append(s)
        for e in range(m):
            if se[e] <= e and (e == m - 1 or se[e + 1] > se[e]) and e + 1 - se[e] >= min_len:
                a, b = se[e], e + 1
                out.append((strand, a, b, q[a:b]) if strand == 0 else (strand, m - b, m - a, q[a:b]))
    return sorted(out)


def _occ(recs, w):
    """sorted (record, offset) of every occurrence of w"""
    out = []
    for i, r in enumerate(recs):
        o = r.find(w)
        while o >= 0:
            out.append((i, o))
            o = r.find(w, o + 1)
    return out


def test_mems_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    for v in ("0", "x", "-1"):
        r = _run("mems", "-i", str(tmp_path / "o"), "--min-len", v, "p.fa")
        assert r.returncode == 1 and "--min-len" in r.stderr
    r = _run("mems", "p.fa")
    assert r.returncode == 1 and "usage" in r.stderr and "mems" in r.stderr
    for opt in (["--mismatches", "1"], ["--best"]):
        r = _run("mems", "-i", str(tmp_path / "o"), *opt, "p.fa")
        assert r.returncode == 1 and "usage" in r.stderr
    r = _run("count", "-i", str(tmp_path / "o"), "--min-len", "5", "p.fa")
    assert r.returncode == 1 and "usage" in r.stderr


@pytest.mark.gpu
def test_mems_end_to_end(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    from debwt_amd import fasta
    fa = os.path.join(GOLDEN, "shared_ends_duplicates.fa")
    recs = ["".join("ACGT"[c] for c in r) for r in fasta.read_fasta(fa)[1]]
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, fa], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", fa)
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(5)
    reads = []
    for i in range(20):
        rec = recs[int(rng.integers(0, len(recs)))]
        L = int(rng.integers(20, 80))
        p = int(rng.integers(0, len(rec) - L))
        s = list(rec[p:p + L])
        for _ in range(int(rng.integers(0, 3))):
            s[int(rng.integers(0, L))] = "ACGTN"[int(rng.integers(0, 5))]
        s = "".join(s)
        if i % 3 == 0:
            s = _revcomp(s)
        if i % 5 == 0:
            rec2 = recs[int(rng.integers(0, len(recs)))]
            s += rec2[:25]
        reads.append(s)
    reads += ["NNNNNNNN", ""]
    pf = tmp_path / "r.fq"
    pf.write_text("".join(f"@r{i}\n{p}\n+\n{'I' * len(p)}\n" for i, p in enumerate(reads)))
    for min_len in (1, 12):
        for both in (False, True):
            for max_hits in (0, 2):
                opts = ["--min-len", str(min_len)] + (["--both-strands"] if both else []) + \
                       (["--max-hits", str(max_hits)] if max_hits else [])
                r = _run("mems", "-i", out, *opts, str(pf))
                assert r.returncode == 0, r.stderr
                want = []
                for i, p in enumerate(reads):
                    for strand, a, b, w in _mems(recs, p, min_len, both):
                        occ = _occ(recs, w)
                        cnt = len(occ)
                        if max_hits:
                            occ = None                        # the first M in suffix order: checked below
                        hits = ",".join(f"{x}:{y}" for x, y in occ) if occ is not None else None
                        want.append((f"r{i}", "+-"[strand], str(a), str(b), str(cnt), hits, w))
                lines = r.stdout.splitlines()
                assert len(lines) == len(want), opts
                for line, w in zip(lines, want):
                    f = line.split("\t")
                    assert f[:5] == list(w[:5]), (opts, line, w)
                    if w[5] is not None:
                        assert f[5] == w[5], (opts, line)
                    else:
                        got = [tuple(map(int, x.split(":"))) for x in f[5].split(",")] if f[5] else []
                        assert len(got) == min(int(w[4]), max_hits) and got == sorted(got)
                        assert set(got) <= set(_occ(recs, w[6])), (opts, line)
    # default min_len 19, and count / locate untouched by the new command
    r = _run("mems", "-i", out, str(pf))
    assert r.returncode == 0 and all(int(x.split("\t")[3]) - int(x.split("\t")[2]) >= 19 for x in r.stdout.splitlines())
    r0 = _run("count", "-i", out, str(pf))
    assert r0.returncode == 0 and all(len(x.split("\t")) == 2 for x in r0.stdout.splitlines())
