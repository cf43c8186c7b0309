"""deBWT-query graph --clean and unitigs --clean (debwt_fm_graph_clean): on the shared read set with errors the cleaned GFA,
the states file and the one unitig against the reference of graph_clean_ref.py, on one strand and on both; the output
without --clean against the reference functions of the graph tests; usage errors."""
import subprocess

import pytest

import graph_clean_ref as gc
from bigraph_ref import doubled, sequences_both, unitigs_both
from overlap_ref import revcomp
from string_graph_ref import Graph, sequences, unitigs
from test_cli_query_bigraph import fasta_both, gfa_both
from test_cli_query_graph import CLI, STATE, _have_query, _run, fasta, gfa

STATES = STATE + ["clipped", "popped"]


def test_clean_usage_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    o = str(tmp_path / "o")
    for args in (["graph", "-i", o, "--clean", "--all-edges"], ["graph", "-i", o, "--max-tip", "2", "--all-edges"],
                 ["graph", "-i", o, "--all-edges", "--clean-rounds", "2"], ["graph", "-i", o, "--max-bubble"],
                 ["count", "-i", o, "--clean", "p.fa"], ["overlaps", "-i", o, "--max-tip", "3", "p.fa"]):
        r = _run(*args)
        assert r.returncode == 1 and "usage" in r.stderr and "--clean-rounds R" in r.stderr and not r.stdout, args
    for args, word in ((["--clean-rounds", "0"], "--clean-rounds"), (["--max-tip", "x"], "--max-tip"),
                       (["--max-bubble", "-1"], "--max-bubble"), (["--max-tip", "0", "--max-bubble", "0"], "both 0")):
        r = _run("unitigs", "-i", o, *args)
        assert r.returncode == 1 and word in r.stderr and not r.stdout, args
    for cmd in ("graph", "unitigs"):
        r = _run(cmd, "-i", str(tmp_path / "missing"), "--clean")              # no OUT.sa
        assert r.returncode == 1 and ".sa" in r.stderr and not r.stdout


class Cleaned:
    """what gfa() and fasta() read, for a cleaned graph"""

    def __init__(self, strs, state, lists, paths, circular, seqs):
        self.strs, self.state, self.I, self.paths, self.circular, self.seqs = strs, state, lists, paths, circular, seqs


@pytest.mark.gpu
def test_clean_end_to_end(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    g, reads = gc.error_reads()
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(reads)))
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, "-k", "32", str(fa)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", str(fa))
    assert r.returncode == 0, r.stderr
    sf = tmp_path / "states.tsv"
    opts = ["--min-overlap", "40"]

    # both strands: the two mirrored halves of the graph are cleaned alike and give the one unitig once
    G = Graph(doubled(reads), 40)
    state, lists, rounds = gc.clean(G.state, G.I, 3, 16, 8, mirrored=True)
    paths, circ = unitigs_both(state, lists)
    C = Cleaned(reads, state, lists, paths, circ, sequences_both(reads, lists, paths, circ))
    r = _run("unitigs", "-i", out, *opts, "--both-strands", "--clean", "--max-tip", "3")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and lines[1] in (g, revcomp(g)) and lines[1] == C.seqs[0]
    assert lines[0] == f">unitig_0 reads={len(paths[0])} len=2000 circular=0 first={paths[0][0] >> 1}{'+-'[paths[0][0] & 1]}"
    assert f"clean: {rounds} rounds, 10 tips of 10 nodes clipped, 2 branches of 12 nodes popped" in r.stderr
    assert "1 unitigs" in r.stderr
    r = _run("graph", "-i", out, *opts, "--both-strands", "--max-tip", "3", "--states", str(sf))     # --max-tip implies --clean
    assert r.returncode == 0, r.stderr
    want = gfa_both(reads, C, lists)
    assert r.stdout.splitlines() == want
    named = sf.read_text().splitlines()
    assert named == [f"{i}\t{STATES[state[2 * i]]}" for i in range(len(reads))]
    assert sum(x.endswith("clipped") for x in named) == 5 and sum(x.endswith("popped") for x in named) == 6
    gone = {str(i) for i in range(len(reads)) if state[2 * i] in (gc.CLIPPED, gc.POPPED)}
    assert len(gone) == 11
    for x in want:
        f = x.split("\t")
        assert not (f[0] == "S" and f[1] in gone) and not (f[0] == "L" and (f[1] in gone or f[3] in gone))
    r = _run("graph", "-i", out, *opts, "--both-strands", "--max-tip", "3", "--max-bubble", "4", "--states", str(sf))
    assert r.returncode == 0, r.stderr
    named = sf.read_text().splitlines()
    assert sum(x.endswith("clipped") for x in named) == 5 and sum(x.endswith("popped") for x in named) == 0

    # one strand of the same index
    F = Graph(reads, 40)
    state, lists, rounds = gc.clean(F.state, F.I, 3, 16, 8)
    paths, circ = unitigs(state, lists)
    C = Cleaned(reads, state, lists, paths, circ, sequences(reads, lists, paths, circ))
    r = _run("graph", "-i", out, *opts, "--clean", "--max-tip", "3", "--states", str(sf))
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == gfa(C, lists)
    named = sf.read_text().splitlines()
    assert named == [f"{i}\t{STATES[s]}" for i, s in enumerate(state)]
    assert sum(x.endswith("clipped") for x in named) == 5 and sum(x.endswith("popped") for x in named) == 6
    r = _run("unitigs", "-i", out, *opts, "--clean", "--max-tip", "3", "--clean-rounds", "8")
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == fasta(C) and "1 unitigs" in r.stderr
    assert r.stdout.splitlines()[1] == g and len(r.stdout.splitlines()) == 2
    assert "clean: 2 rounds, 5 tips of 5 nodes clipped, 1 branches of 6 nodes popped" in r.stderr

    # without --clean: what the commands wrote before
    r = _run("graph", "-i", out, *opts, "--states", str(sf))
    assert r.returncode == 0 and r.stdout.splitlines() == gfa(F, F.I) and "clean:" not in r.stderr
    assert sf.read_text().splitlines() == [f"{i}\t{STATE[s]}" for i, s in enumerate(F.state)]
    r = _run("unitigs", "-i", out, *opts)
    assert r.returncode == 0 and r.stdout.splitlines() == fasta(F) and len(F.paths) > 1
    r = _run("graph", "-i", out, *opts, "--both-strands")
    assert r.returncode == 0 and r.stdout.splitlines() == gfa_both(reads, G, G.I)
    r = _run("unitigs", "-i", out, *opts, "--both-strands")
    lines, nu = fasta_both(reads, G)
    assert r.returncode == 0 and r.stdout.splitlines() == lines and nu == 14
