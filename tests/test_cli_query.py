"""deBWT-query (cli/query.c): index / count / locate over the files deBWT writes, against a numpy search of the text."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(*args):
    return subprocess.run([QUERY, *args], capture_output=True, text=True, timeout=300)


def test_query_usage_and_argument_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    r = _run()
    assert r.returncode == 1 and "usage" in r.stderr
    r = _run("search", "-i", "x", "p.fa")
    assert r.returncode == 1 and "usage" in r.stderr
    r = _run("count", "p.fa")                                            # no -i
    assert r.returncode == 1 and "usage" in r.stderr
    r = _run("count", "-i", str(tmp_path / "o"))                         # no pattern file
    assert r.returncode == 1 and "usage" in r.stderr
    r = _run("index", "-i", str(tmp_path / "o"), "--sa", "3", "x.fa")
    assert r.returncode == 1 and "power of two" in r.stderr
    r = _run("index", "-i", str(tmp_path / "o"), "--sa", "2048", "x.fa")
    assert r.returncode == 1 and "power of two" in r.stderr
    r = _run("index", "-i", str(tmp_path / "o"), "-t", "zero", "x.fa")
    assert r.returncode == 1 and "thread number" in r.stderr
    r = _run("count", "-i", str(tmp_path / "o"), "--max-hits", "3", "p.fa")   # a locate option
    assert r.returncode == 1 and "usage" in r.stderr
    r = _run("locate", "-i", str(tmp_path / "o"), "--max-hits", "many", "p.fa")
    assert r.returncode == 1 and "--max-hits" in r.stderr
    (tmp_path / "p.fa").write_text(">p\nACGT\n")
    r = _run("count", "-i", str(tmp_path / "missing"), str(tmp_path / "p.fa"))   # no OUT.sa
    assert r.returncode == 1 and "OUT.sa" not in r.stdout and r.stdout == ""
    (tmp_path / "bad.fa").write_text("ACGT\n")
    r = _run("count", "-i", str(tmp_path / "missing"), str(tmp_path / "bad.fa"))
    assert r.returncode == 1 and "not FASTA or FASTQ" in r.stderr


def _naive(recs, pat):
    """(record, offset) of every occurrence of pat inside a record, ascending"""
    hits = []
    for i, r in enumerate(recs):
        s = r.upper()
        p = pat.upper()
        start = s.find(p)
        while start >= 0:
            hits.append((i, start))
            start = s.find(p, start + 1)
    return hits


@pytest.mark.gpu
def test_query_end_to_end(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    from debwt_amd import fasta
    fa = os.path.join(GOLDEN, "shared_ends_duplicates.fa")
    other = os.path.join(GOLDEN, "special_branches.fa")
    recs = ["".join("ACGT"[c] for c in r) for r in fasta.read_fasta(fa)[1]]
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, fa], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", fa)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(out + ".sa")
    rng = np.random.default_rng(1)
    pats = []
    for i in range(60):
        rec = recs[int(rng.integers(0, len(recs)))]
        L = int(rng.integers(1, 40))
        p = int(rng.integers(0, len(rec) - L))
        s = rec[p:p + L]
        if i % 5 == 0:
            s = s.lower()
        pats.append(s)
    pats += ["ACGTN", "", "TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT"]
    pf = tmp_path / "p.fa"
    pf.write_text("".join(f">q{i} some description\n{p[:20]}\n{p[20:]}\n" for i, p in enumerate(pats)))
    qf = tmp_path / "p.fq"
    qf.write_text("".join(f"@q{i}\n{p}\n+\n{'I' * len(p)}\n" for i, p in enumerate(pats)))
    for f in (pf, qf):
        r = _run("count", "-i", out, str(f))
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(pats)
        for i, (line, p) in enumerate(zip(lines, pats)):
            name, cnt = line.split("\t")
            want = len(_naive(recs, p)) if p and set(p.upper()) <= set("ACGT") else 0
            assert name == f"q{i}" and int(cnt) == want, (p, line)
    r = _run("locate", "-i", out, str(qf))
    assert r.returncode == 0, r.stderr
    for line, p in zip(r.stdout.splitlines(), pats):
        name, cnt, hits = line.split("\t")
        want = _naive(recs, p) if p and set(p.upper()) <= set("ACGT") else []
        assert int(cnt) == len(want)
        assert hits == ",".join(f"{a}:{b}" for a, b in want), (p, line)
    r = _run("locate", "-i", out, "--max-hits", "2", str(qf))
    assert r.returncode == 0, r.stderr
    for line, p in zip(r.stdout.splitlines(), pats):
        name, cnt, hits = line.split("\t")
        want = _naive(recs, p) if p and set(p.upper()) <= set("ACGT") else []
        got = [tuple(int(x) for x in h.split(":")) for h in hits.split(",")] if hits else []
        assert int(cnt) == len(want) and len(got) == min(2, len(want)) and set(got) <= set(want)
        assert got == sorted(got)
    # OUT is not the BWT of another FASTA: exit 1, and a header that does not match OUT is refused
    r = _run("index", "-i", out, other)
    assert r.returncode == 1 and "not the BWT" in r.stderr
    out2 = str(tmp_path / "out2")
    r = subprocess.run([CLI, "-o", out2, other], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    os.replace(out + ".sa", out2 + ".sa")
    r = _run("count", "-i", out2, str(pf))
    assert r.returncode == 1 and "does not belong" in r.stderr
