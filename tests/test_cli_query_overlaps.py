"""deBWT-query overlaps (debwt_fm_overlaps): option errors without a GPU; on the GPU, deBWT, index and overlaps on a FASTA
of the synthetic read set, queried with itself, with --both-strands, --longest and --no-self, line by line against the
reference of overlap_ref.py."""
import os
import subprocess

import pytest

from conftest import ROOT
from overlap_ref import CONTAINS, WHOLE, Ref, longest_of, synthetic_reads

CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(*args):
    return subprocess.run([QUERY, *args], capture_output=True, text=True, timeout=300)


def test_overlaps_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    for v in ("0", "x", "-1"):
        r = _run("overlaps", "-i", str(tmp_path / "o"), "--min-overlap", v, "p.fa")
        assert r.returncode == 1 and "--min-overlap" in r.stderr
    r = _run("overlaps", "p.fa")
    assert r.returncode == 1 and "usage" in r.stderr and "overlaps" in r.stderr
    for opt in (["--mismatches", "1"], ["--best"], ["--min-len", "5"], ["--max-hits", "3"]):
        r = _run("overlaps", "-i", str(tmp_path / "o"), *opt, "p.fa")
        assert r.returncode == 1 and "usage" in r.stderr
    for cmd in ("count", "mems"):
        r = _run(cmd, "-i", str(tmp_path / "o"), "--min-overlap", "5", "p.fa")
        assert r.returncode == 1 and "usage" in r.stderr
        for opt in ("--longest", "--no-self"):
            r = _run(cmd, "-i", str(tmp_path / "o"), opt, "p.fa")
            assert r.returncode == 1 and "usage" in r.stderr


@pytest.mark.gpu
def test_overlaps_end_to_end(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    strs = synthetic_reads()
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(strs)))
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, str(fa)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", str(fa))
    assert r.returncode == 0, r.stderr
    names = {0: ".", CONTAINS: "C", WHOLE: "W", CONTAINS | WHOLE: "CW"}
    for min_overlap, both, longest, no_self in ((20, False, False, False), (20, True, True, True), (33, True, False, True),
                                                (None, False, True, False)):
        opts = (["--min-overlap", str(min_overlap)] if min_overlap else []) + (["--both-strands"] if both else []) + \
               (["--longest"] if longest else []) + (["--no-self"] if no_self else [])
        r = _run("overlaps", "-i", out, *opts, str(fa))
        assert r.returncode == 0, r.stderr
        R = Ref(strs, min_overlap or 20)                      # 20 is the default
        want = []
        for i, p in enumerate(strs):
            hits = R.both(p) if both else R.hits(p)
            if longest:
                hits = longest_of(hits)
            for j, L, strand, fl in hits:
                if no_self and strand == 0 and j == i and L == len(p):
                    continue
                want.append(f"r{i}\t{'+-'[strand]}\t{j}\t{L}\t{names[fl]}")
        lines = r.stdout.splitlines()
        assert len(lines) == len(want), opts
        for got, w in zip(lines, want):
            assert got == w, opts
        assert len(want) > len(strs)
    # the other subcommands are untouched by the new one
    r0 = _run("count", "-i", out, str(fa))
    assert r0.returncode == 0 and all(len(x.split("\t")) == 2 for x in r0.stdout.splitlines())
