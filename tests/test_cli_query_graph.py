"""deBWT-query graph and unitigs (debwt_fm_string_graph, debwt_fm_unitigs, debwt_fm_extract): after index, the GFA lines, the
states file and the unitig FASTA of a read set against the reference of string_graph_ref.py, on a tiling and on the
synthetic read set; --all-edges, --states and the error exits."""
import os
import subprocess

import pytest

from conftest import ROOT
from overlap_ref import synthetic_reads
from string_graph_ref import Graph, tiling

CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")
STATE = ["kept", "duplicate", "contained"]


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(*args):
    return subprocess.run([QUERY, *args], capture_output=True, text=True, timeout=300)


def gfa(G, lists):
    out = ["H\tVN:Z:1.0"]
    out += [f"S\t{i}\t*\tLN:i:{len(s)}" for i, s in enumerate(G.strs) if G.state[i] == 0]
    out += [f"L\t{i}\t+\t{k}\t+\t{L}M" for i, l in enumerate(lists) for k, L in l]
    return out


def fasta(G):
    out = []
    for u, (p, c, s) in enumerate(zip(G.paths, G.circular, G.seqs)):
        out += [f">unitig_{u} reads={len(p)} len={len(s)} circular={c} first={p[0]}", s]
    return out


def test_graph_usage_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    o = str(tmp_path / "o")
    for args in (["graph"], ["graph", "-i", o, "reads.fa"], ["unitigs", "-i", o, "--all-edges"], ["graph", "-i", o, "--longest"],
                 ["unitigs", "-i", o, "x"], ["count", "-i", o, "--states", "s.txt", "p.fa"]):
        r = _run(*args)
        assert r.returncode == 1 and "usage" in r.stderr and "unitigs" in r.stderr and not r.stdout, args
    r = _run("graph", "-i", o, "--min-overlap", "0")
    assert r.returncode == 1 and "--min-overlap" in r.stderr and not r.stdout
    for cmd in ("graph", "unitigs"):
        r = _run(cmd, "-i", str(tmp_path / "missing"))                      # no OUT.sa
        assert r.returncode == 1 and ".sa" in r.stderr and not r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("name,min_overlap", [("tiling", 30), ("synthetic", 20)])
def test_graph_and_unitigs_end_to_end(tmp_path, name, min_overlap):
    assert _have_query(), "cli/deBWT-query is not built"
    strs = tiling(1, 2000, 60, 5)[1] if name == "tiling" else synthetic_reads()
    G = Graph(strs, min_overlap)
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(strs)))
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, "-k", "32", str(fa)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", str(fa))
    assert r.returncode == 0, r.stderr
    sf = tmp_path / "states.tsv"
    r = _run("graph", "-i", out, "--min-overlap", str(min_overlap), "--states", str(sf))
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == gfa(G, G.I)
    assert sf.read_text().splitlines() == [f"{i}\t{STATE[s]}" for i, s in enumerate(G.state)]
    assert f"{G.state.count(0)} kept" in r.stderr and f"{sum(len(l) for l in G.E)} edges" in r.stderr
    r = _run("graph", "-i", out, "--min-overlap", str(min_overlap), "--all-edges")
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == gfa(G, G.E) and len(gfa(G, G.E)) > len(gfa(G, G.I))
    r = _run("unitigs", "-i", out, "--min-overlap", str(min_overlap))
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == fasta(G)
    assert f"{len(G.paths)} unitigs" in r.stderr
    r = _run("graph", "-i", out, "--states", str(tmp_path / "no" / "dir.tsv"))
    assert r.returncode == 1 and "dir.tsv" in r.stderr and not r.stdout
