"""deBWT-query kmers and correct (debwt_fm_kmer_counts, debwt_fm_correct): option errors without a GPU; on the GPU, deBWT,
index and both subcommands on a FASTA of the seeded read set -- kmers against the reference of kmer_ref.py, correct
against FMIndex.correct on the same index files."""
import os
import subprocess

import numpy as np
import pytest

import kmer_ref as KR
from conftest import ROOT

CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(*args):
    return subprocess.run([QUERY, *args], capture_output=True, text=True, timeout=300)


def test_kmers_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    o = str(tmp_path / "o")
    for cmd in ("kmers", "correct"):
        r = _run(cmd, "-i", o, "p.fa")                          # -k is required
        assert r.returncode == 1 and "-k" in r.stderr
        for v in ("0", "x", "-3"):
            r = _run(cmd, "-i", o, "-k", v, "p.fa")
            assert r.returncode == 1 and "-k" in r.stderr
        r = _run(cmd, "-k", "15", "p.fa")
        assert r.returncode == 1 and "usage" in r.stderr and "kmers" in r.stderr and "correct" in r.stderr
    for opt in (["--min-count", "0"], ["--rounds", "0"], ["--rounds", "17"]):
        r = _run("correct", "-i", o, "-k", "15", *opt, "p.fa")
        assert r.returncode == 1 and opt[0] in r.stderr
    for opt in (["--min-count", "2"], ["--rounds", "2"], ["--forward"], ["--report", "x"]):
        r = _run("kmers", "-i", o, "-k", "15", *opt, "p.fa")
        assert r.returncode == 1 and "usage" in r.stderr
    r = _run("correct", "-i", o, "-k", "15", "--both-strands", "p.fa")
    assert r.returncode == 1 and "usage" in r.stderr
    for cmd in ("count", "locate", "mems", "overlaps", "map", "index", "extract"):     # -k does not slip into other modes
        r = _run(cmd, "-i", o, "-k", "15", "p.fa")
        assert r.returncode == 1 and "usage" in r.stderr
        r = _run(cmd, "-i", o, "--min-count", "3", "p.fa")
        assert r.returncode == 1 and "usage" in r.stderr


@pytest.mark.gpu
def test_kmers_and_correct_end_to_end(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    from debwt_amd import api
    strs = KR.read_set()["records"]
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(f">r{i} a comment\n{s}\n" for i, s in enumerate(strs)))
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, str(fa)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", str(fa))
    assert r.returncode == 0, r.stderr
    k = 15
    pats = KR.correction_queries(k)
    q = tmp_path / "q.fa"
    q.write_text("".join(f">q{i}\n{s}\n" for i, s in enumerate(pats)))
    for both in (False, True):
        r = _run("kmers", "-i", out, "-k", str(k), *(["--both-strands"] if both else []), str(q))
        assert r.returncode == 0, r.stderr
        R = KR.ref_of(k, both)
        lines = r.stdout.splitlines()
        assert len(lines) == len(pats)
        for i, (ln, p) in enumerate(zip(lines, pats)):
            name, col = ln.split("\t")
            assert name == f"q{i}"
            assert col == ("*" if len(p) < k else ",".join(str(c) for c in R.profile(p))), i
    # correct: FASTA and report against FMIndex.correct on an index opened from the same files
    words = np.fromfile(out, dtype=np.uint64)
    hrows = np.fromfile(out + ".#", dtype=np.uint64)
    drow = int(np.fromfile(out + ".$", dtype=np.uint64)[0])
    sa = np.fromfile(out + ".sa", dtype=np.uint64)
    fm = api.FMIndex.open(words, int(sa[1]), hrows, drow, sa[16:], sa_sample=int(sa[3]))
    status = {api.CORRECT_SHORT: "short", api.CORRECT_CLEAN: "clean", api.CORRECT_FIXED: "fixed", api.CORRECT_WEAK: "weak"}
    for opts, kw in (([], {}), (["--min-count", "2", "--rounds", "1", "--forward"], {"min_count": 2, "rounds": 1, "strands": "forward"})):
        rep = tmp_path / "report.tsv"
        r = _run("correct", "-i", out, "-k", str(k), *opts, "--report", str(rep), str(q))
        assert r.returncode == 0, r.stderr
        reads, info = fm.correct(pats, k, **kw)
        want = "".join(f">q{i}\n{s.decode()}\n" for i, s in enumerate(reads))
        assert r.stdout == want
        rows = [ln.split("\t") for ln in rep.read_text().splitlines()]
        assert rows == [[f"q{i}", status[int(x["flags"])], str(x["fixes"]), str(x["weak_before"]), str(x["weak_after"])]
                        for i, x in enumerate(info)]
        assert len(r.stderr.strip().splitlines()) == 1 and f"{int(info['fixes'].sum())} fixes" in r.stderr
        assert int(info["fixes"].sum()) > 0
    fm.close()
