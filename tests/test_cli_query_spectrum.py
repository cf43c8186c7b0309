"""deBWT-query spectrum and correct --min-count auto (debwt_fm_spectrum, debwt_fm_kmer_list): option errors without a GPU;
on the GPU, deBWT, index and spectrum on a FASTA of the seeded read set -- header lines, histogram rows and the --list
file against spectrum_ref.py -- and correct --min-count auto byte for byte against correct --min-count V."""
import os
import subprocess

import numpy as np
import pytest

import kmer_ref as KR
import spectrum_ref as SR
from conftest import ROOT

CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(*args):
    return subprocess.run([QUERY, *args], capture_output=True, text=True, timeout=300)


def test_spectrum_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    o = str(tmp_path / "o")
    r = _run("spectrum", "-i", o)                                # -k is required
    assert r.returncode == 1 and "-k" in r.stderr and "usage" in r.stderr and "spectrum" in r.stderr
    for v in ("0", "33", "x", "-3"):
        r = _run("spectrum", "-i", o, "-k", v)
        assert r.returncode == 1 and "-k" in r.stderr and "usage" not in r.stderr
    for v in ("1", "4097", "0", "x"):
        r = _run("spectrum", "-i", o, "-k", "21", "--bins", v)
        assert r.returncode == 1 and "--bins" in r.stderr
    for opt in ("--at-least", "--at-most"):
        for v in ("0", "x", "4294967296"):
            r = _run("spectrum", "-i", o, "-k", "21", "--list", "l.tsv", opt, v)
            assert r.returncode == 1 and opt in r.stderr
    r = _run("spectrum", "-i", o, "-k", "21", "--list", "l.tsv", "--at-least", "9", "--at-most", "8")
    assert r.returncode == 1 and "--at-least" in r.stderr and "--at-most" in r.stderr
    for opt in (["--at-least", "2"], ["--at-most", "9"], ["--at-least", "2", "--at-most", "9"]):
        r = _run("spectrum", "-i", o, "-k", "21", *opt)          # filters without --list
        assert r.returncode == 1 and "--list" in r.stderr
    r = _run("spectrum", "-k", "21")                             # -i is required
    assert r.returncode == 1 and "usage" in r.stderr
    r = _run("spectrum", "-i", o, "-k", "21", "reads.fa")        # no file argument
    assert r.returncode == 1 and "usage" in r.stderr
    for opt in (["--both-strands"], ["--min-count", "3"], ["--rounds", "2"], ["--report", "x"]):
        r = _run("spectrum", "-i", o, "-k", "21", *opt)
        assert r.returncode == 1 and "usage" in r.stderr
    # the options of spectrum do not slip into the other subcommands
    for cmd in ("count", "locate", "mems", "overlaps", "map", "index", "extract", "kmers", "correct", "graph", "unitigs",
                "pileup", "consensus"):
        for opt in (["--bins", "64"], ["--list", "l.tsv"], ["--at-least", "2"], ["--at-most", "9"]):
            r = _run(cmd, "-i", o, *(["-k", "15"] if cmd in ("kmers", "correct") else []), *opt, "p.fa")
            assert r.returncode == 1 and "usage" in r.stderr, (cmd, opt)
    r = _run("correct", "-i", o, "-k", "15", "--min-count", "automatic", "p.fa")
    assert r.returncode == 1 and "--min-count" in r.stderr
    r = _run("kmers", "-i", o, "-k", "15", "--min-count", "auto", "p.fa")
    assert r.returncode == 1 and "usage" in r.stderr


def _spectrum_lines(D, k, strands, bins):
    hist = SR.histogram(D, bins)
    distinct, total, _ = SR.totals(D, bins)
    valley, peak, est = SR.threshold(hist, total)
    head = [f"# k\t{k}", f"# strands\t{strands}", f"# distinct\t{distinct}", f"# total\t{total}", f"# valley\t{valley}",
            f"# peak\t{peak}", f"# est_size\t{est}"]
    rows = [f"{'>=' if c == bins - 1 else ''}{c}\t{h}" for c, h in enumerate(hist) if h]
    return head + rows


@pytest.mark.gpu
def test_spectrum_end_to_end(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    strs = KR.read_set()["records"]
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(f">r{i} a comment\n{s}\n" for i, s in enumerate(strs)))
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, str(fa)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", str(fa))
    assert r.returncode == 0, r.stderr
    lst = tmp_path / "list.tsv"
    for k, opts, strands, bins, lo, hi in ((21, [], "both", 256, 1, SR.U32_MAX),
                                           (15, ["--forward", "--bins", "16", "--at-least", "3"], "forward", 16, 3, SR.U32_MAX),
                                           (4, ["--bins", "2", "--at-least", "200", "--at-most", "900"], "both", 2, 200, 900),
                                           (32, ["--forward", "--at-most", "1"], "forward", 256, 1, 1)):
        D = SR.of_read_set(k, strands == "both")
        r = _run("spectrum", "-i", out, "-k", str(k), "--list", str(lst), *opts)
        assert r.returncode == 0, r.stderr
        assert r.stdout.splitlines() == _spectrum_lines(D, k, strands, bins)
        assert lst.read_text().splitlines() == [f"{SR.string_of(c, k)}\t{m}" for c, m in SR.listing(D, lo, hi)]
        assert len(r.stderr.strip().splitlines()) == 1 and "spectrum:" in r.stderr
    lst.unlink()
    r = _run("spectrum", "-i", out, "-k", "1")                   # single bases: the histogram only falls
    assert r.returncode == 0 and r.stdout.splitlines() == _spectrum_lines(SR.of_read_set(1, True), 1, "both", 256)
    assert "# valley\t0" in r.stdout and "no valley" in r.stderr and not lst.exists()
    # correct --min-count auto: the valley, named on stderr, and the same bytes as with the number
    pats = KR.correction_queries(15)
    q = tmp_path / "q.fa"
    q.write_text("".join(f">q{i}\n{s}\n" for i, s in enumerate(pats)))
    for k, opts, both in ((15, [], True), (21, ["--rounds", "2"], True), (15, ["--forward"], False)):
        D = SR.of_read_set(k, both)
        valley = SR.threshold(SR.histogram(D, 256), SR.totals(D, 256)[1])[0]
        assert valley > 0
        ra, rv = tmp_path / "auto.tsv", tmp_path / "value.tsv"
        a = _run("correct", "-i", out, "-k", str(k), *opts, "--min-count", "auto", "--report", str(ra), str(q))
        v = _run("correct", "-i", out, "-k", str(k), *opts, "--min-count", str(valley), "--report", str(rv), str(q))
        assert a.returncode == 0 and v.returncode == 0, a.stderr + v.stderr
        assert a.stdout == v.stdout and len(a.stdout) > 0 and ra.read_bytes() == rv.read_bytes()
        err = a.stderr.strip().splitlines()
        assert len(err) == 2 and f"--min-count auto: {valley} " in err[0]
        assert err[1].rsplit(",", 1)[0] == v.stderr.strip().rsplit(",", 1)[0]          # the summary line, without its ms
    # a collection without a valley: exit status 1 and a message
    fa1 = tmp_path / "single.fa"
    rng = np.random.default_rng(17)
    fa1.write_text("".join(f">s{i}\n{KR.rand_dna(rng, 60)}\n" for i in range(40)))
    out1 = str(tmp_path / "single")
    r = subprocess.run([CLI, "-o", out1, str(fa1)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert _run("index", "-i", out1, str(fa1)).returncode == 0
    r = _run("correct", "-i", out1, "-k", "15", "--min-count", "auto", str(fa1))
    assert r.returncode == 1 and r.stdout == "" and "no valley" in r.stderr
