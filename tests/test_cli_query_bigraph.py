"""deBWT-query graph --both-strands and unitigs --both-strands (debwt_fm_string_graph_both, debwt_fm_unitigs_both): the GFA
lines, the states file and the unitig FASTA of a stranded read set with crafted corners against the reference on the
doubled collection, line by line; the same commands without the option against the strand-0 reference; usage errors."""
import os
import subprocess

import pytest

from bigraph_ref import crafted, doubled, is_selfrc, sequences_both, stranded, unitigs_both
from conftest import ROOT
from overlap_ref import synthetic_reads
from string_graph_ref import Graph
from test_cli_query_graph import CLI, QUERY, STATE, _have_query, _run, fasta, gfa


def mirror_node(state, v):
    return v if is_selfrc(state, v) else v ^ 1


def gfa_both(strs, G, lists):
    """one S line per kept read; an edge u -> v is written iff (u, v) <= (mirror v, mirror u)"""
    out = ["H\tVN:Z:1.0"]
    out += [f"S\t{r}\t*\tLN:i:{len(s)}" for r, s in enumerate(strs) if G.state[2 * r] == 0]
    for u, l in enumerate(lists):
        for v, L in l:
            if (u, v) <= (mirror_node(G.state, v), mirror_node(G.state, u)):
                out.append(f"L\t{u >> 1}\t{'+-'[u & 1]}\t{v >> 1}\t{'+-'[v & 1]}\t{L}M")
    return out


def fasta_both(strs, G):
    paths, circ = unitigs_both(G.state, G.I)
    out = []
    for u, (p, c, s) in enumerate(zip(paths, circ, sequences_both(strs, G.I, paths, circ))):
        out += [f">unitig_{u} reads={len(p)} len={len(s)} circular={c} first={p[0] >> 1}{'+-'[p[0] & 1]}", s]
    return out, len(paths)


def test_both_strands_usage_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    o = str(tmp_path / "o")
    for args in (["graph", "-i", o, "--both-strands", "reads.fa"], ["unitigs", "-i", o, "--both-strands", "--all-edges"],
                 ["extract", "-i", o, "--both-strands", "--all"], ["correct", "-i", o, "-k", "21", "--both-strands", "r.fa"]):
        r = _run(*args)
        assert r.returncode == 1 and "usage" in r.stderr and "--both-strands] [--states" in r.stderr and not r.stdout, args
    for cmd in ("graph", "unitigs"):
        r = _run(cmd, "-i", str(tmp_path / "missing"), "--both-strands")       # no OUT.sa
        assert r.returncode == 1 and ".sa" in r.stderr and not r.stdout
    r = _run("graph", "-i", o, "--both-strands", "--min-overlap", "0")
    assert r.returncode == 1 and "--min-overlap" in r.stderr and not r.stdout


@pytest.mark.gpu
def test_both_strands_end_to_end(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    strs = crafted(stranded(synthetic_reads(), 7))[0]
    G = Graph(doubled(strs), 20)
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(strs)))
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, "-k", "32", str(fa)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", str(fa))
    assert r.returncode == 0, r.stderr
    sf = tmp_path / "states.tsv"
    r = _run("graph", "-i", out, "--both-strands", "--states", str(sf))
    assert r.returncode == 0, r.stderr
    want = gfa_both(strs, G, G.I)
    assert r.stdout.splitlines() == want
    assert sf.read_text().splitlines() == [f"{i}\t{STATE[G.state[2 * i]]}" for i in range(len(strs))]
    assert f"{G.state[0::2].count(0)} kept" in r.stderr and f"{sum(len(l) for l in G.E)} edges" in r.stderr
    assert f"{sum(1 for x in want if x[0] == 'L')} written" in r.stderr
    assert any(x.split("\t")[2] != x.split("\t")[4] for x in want if x[0] == "L")      # links between the strands
    r = _run("graph", "-i", out, "--both-strands", "--all-edges")
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == gfa_both(strs, G, G.E) and len(gfa_both(strs, G, G.E)) > len(want)
    r = _run("unitigs", "-i", out, "--both-strands")
    assert r.returncode == 0, r.stderr
    lines, nu = fasta_both(strs, G)
    assert r.stdout.splitlines() == lines and f"{nu} unitigs" in r.stderr
    assert any(x.endswith("-") for x in lines[0::2]) and any(x.endswith("+") for x in lines[0::2])
    # without the option: the strand-0 graph of the same index, as before
    F = Graph(strs, 20)
    r = _run("graph", "-i", out)
    assert r.returncode == 0 and r.stdout.splitlines() == gfa(F, F.I)
    r = _run("unitigs", "-i", out)
    assert r.returncode == 0 and r.stdout.splitlines() == fasta(F)
