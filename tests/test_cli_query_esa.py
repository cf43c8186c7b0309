"""deBWT-query lcp (debwt_fm_esa_build): option errors without a GPU; on the GPU, deBWT, index and lcp on a FASTA of the
seeded read set -- the three array files, the header line and the profile rows against esa_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import esa_ref as ER
import kmer_ref as KR
from conftest import ROOT

CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")
OTHERS = ("count", "locate", "mems", "overlaps", "map", "index", "extract", "kmers", "correct", "graph", "unitigs", "pileup",
          "consensus", "spectrum")


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(*args):
    return subprocess.run([QUERY, *args], capture_output=True, text=True, timeout=300)


def test_lcp_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    o = str(tmp_path / "o")
    r = _run("lcp")                                              # -i is required
    assert r.returncode == 1 and "usage" in r.stderr and "deBWT-query lcp" in r.stderr
    r = _run("lcp", "-i", o, "reads.fa")                         # no file argument
    assert r.returncode == 1 and "usage" in r.stderr
    for v in ("0", "x", "-3", "4294967296"):
        r = _run("lcp", "-i", o, "--max-lcp", v)
        assert r.returncode == 1 and "--max-lcp" in r.stderr and "usage" not in r.stderr
    for v in ("0", "x", "-1", "4097"):
        r = _run("lcp", "-i", o, "--profile", v)
        assert r.returncode == 1 and "--profile" in r.stderr and "usage" not in r.stderr
    r = _run("lcp", "-i", o, "--max-lcp", "7", "--profile", "8")  # the profile is exact up to the cap only
    assert r.returncode == 1 and "--profile" in r.stderr and "--max-lcp" in r.stderr
    for opt in ("--lcp", "--sa", "--da", "--profile", "--max-lcp"):
        r = _run("lcp", "-i", o, opt)                            # a value is missing
        assert r.returncode == 1 and "usage" in r.stderr
    for opt in (["--both-strands"], ["-k", "21"], ["--bins", "16"], ["--min-overlap", "20"], ["--all"], ["-t", "4"]):
        r = _run("lcp", "-i", o, *opt)                           # the options of the others are none of lcp's
        assert r.returncode == 1 and "usage" in r.stderr, opt
    # the options of lcp do not slip into the other subcommands (--sa is index's own option, with a number)
    for cmd in OTHERS:
        need = ["-k", "15"] if cmd in ("kmers", "correct", "spectrum") else []
        for opt in (["--max-lcp", "64"], ["--lcp", "l.bin"], ["--da", "d.bin"], ["--profile", "8"], ["--sa", "s.bin"]):
            r = _run(cmd, "-i", o, *need, *opt, *([] if cmd == "spectrum" else ["p.fa"]))
            assert r.returncode == 1, (cmd, opt)
            assert ("usage" in r.stderr) != (cmd == "index" and opt[0] == "--sa"), (cmd, opt)
    assert len(OTHERS) == 14


@pytest.mark.gpu
def test_lcp_end_to_end(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    strs = KR.read_set()["records"]
    E = ER.of_read_set()
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(f">r{i} a comment\n{s}\n" for i, s in enumerate(strs)))
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, str(fa)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", str(fa))
    assert r.returncode == 0, r.stderr

    def header(max_lcp):
        sm = E.summary(max_lcp)
        a, b = E.resolve(sm["pos_prev"]), E.resolve(sm["pos"])
        return (f"# n={E.n}\tmax={sm['max']}\tmax_row={sm['max_row']}\tprev={a[0]}:{a[1]}\tpos={b[0]}:{b[1]}"
                f"\tmean={sm['sum'] / E.n:.6f}")

    lf, sf, df = tmp_path / "lcp.bin", tmp_path / "sa.bin", tmp_path / "da.bin"
    r = _run("lcp", "-i", out, "--lcp", str(lf), "--sa", str(sf), "--da", str(df), "--profile", "32")
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(lf, dtype="<u4"), E.lcp())
    assert np.array_equal(np.fromfile(sf, dtype="<u8"), E.sa.astype(np.uint64))
    assert np.array_equal(np.fromfile(df, dtype="<u4"), E.da)
    lines = r.stdout.splitlines()
    assert lines[0] == header(0) and lines[1:] == [f"{k}\t{d}" for k, d in enumerate(E.profile(32), 1)]
    assert len(r.stderr.strip().splitlines()) == 1 and r.stderr.startswith("lcp:")
    for f in (lf, sf, df):
        f.unlink()
    r = _run("lcp", "-i", out, "--max-lcp", "12", "--lcp", str(lf), "--profile", "12")      # capped, the LCP file alone
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(lf, dtype="<u4"), E.lcp(12)) and not sf.exists() and not df.exists()
    assert r.stdout.splitlines() == [header(12)] + [f"{k}\t{d}" for k, d in enumerate(E.profile(12, 12), 1)]
    r = _run("lcp", "-i", out)                                   # no file, no profile: the header line
    assert r.returncode == 0 and r.stdout.splitlines() == [header(0)]
    r = _run("lcp", "-i", out, "--lcp", str(tmp_path / "no" / "dir.bin"))
    assert r.returncode == 1 and "cannot write" in r.stderr and r.stdout == ""
