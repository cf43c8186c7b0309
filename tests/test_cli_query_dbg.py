"""deBWT-query dbg (debwt_fm_cdbg): option errors without a GPU; on the GPU, deBWT, index and dbg on a FASTA of one builder
case and of the small pan-genome -- every S and L line against cdbg_ref.py, --fasta against the same strings, and the
k-mers of every S string through deBWT-query count, whose counts sum to the KC tag."""
import os
import subprocess

import pytest

import cdbg_ref as CR
import esa_ref as ER
import fm_definition as F
from conftest import ROOT
from test_fm_cdbg_ref import pan_genome

CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(*args):
    return subprocess.run([QUERY, *args], capture_output=True, text=True, timeout=300)


def test_dbg_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    o = str(tmp_path / "o")
    r = _run("dbg")                                              # -i is required
    assert r.returncode == 1 and "usage" in r.stderr and "deBWT-query dbg" in r.stderr
    r = _run("dbg", "-k", "21")
    assert r.returncode == 1 and "usage" in r.stderr
    r = _run("dbg", "-i", o)                                     # -k is required
    assert r.returncode == 1 and "-k" in r.stderr
    r = _run("dbg", "-i", o, "-k", "21", "reads.fa")             # no file argument
    assert r.returncode == 1 and "usage" in r.stderr
    for v in ("0", "x", "-3", "4294967295", "4294967296", "21x"):
        r = _run("dbg", "-i", o, "-k", v)
        assert r.returncode == 1 and "-k" in r.stderr and "usage" not in r.stderr, v
    r = _run("dbg", "-i", o, "-k")                               # a value is missing
    assert r.returncode == 1 and "usage" in r.stderr
    for opt in (["--both-strands"], ["--min-len", "20"], ["--min-overlap", "20"], ["--max-lcp", "30"], ["--forward"], ["--seq"],
                ["--min-mapq", "3"], ["--bins", "8"], ["--all-edges"], ["--clean"], ["--states", "s.txt"]):
        r = _run("dbg", "-i", o, "-k", "21", *opt)               # the options of the others are none of dbg's
        assert r.returncode == 1 and "usage" in r.stderr, opt
    for cmd in ("lcp", "repeats", "mums", "graph", "unitigs", "spectrum"):   # and --fasta is none of theirs
        need = ["-k", "15"] if cmd == "spectrum" else []
        r = _run(cmd, "-i", o, *need, "--fasta")
        assert r.returncode == 1 and "usage" in r.stderr, cmd
    r = _run("dbg", "-i", o, "-k", "21")                         # no such index: refused before anything is built
    assert r.returncode == 1 and r.stdout == ""
    r = _run("dbg", "-i", o, "-k", "4294967294", "--fasta")      # the largest k passes the options
    assert r.returncode == 1 and r.stdout == "" and "k-mer length" not in r.stderr and "usage" not in r.stderr


def _indexed(tmp_path, strs, tag):
    fa = tmp_path / f"{tag}.fa"
    fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(strs)))
    out = str(tmp_path / tag)
    r = subprocess.run([CLI, "-o", out, str(fa)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", str(fa))
    assert r.returncode == 0, r.stderr
    return out


def _gfa(G):
    out = ["H\tVN:Z:1.0"]
    for i, (s, u) in enumerate(zip(G.strings(), G.unitigs)):
        out.append(f"S\t{i}\t{s}\tLN:i:{len(s)}\tKC:i:{int(u['kmer_count'])}" + ("\tCL:Z:circular" if u["flags"] & CR.CIRCULAR else ""))
    out += [f"L\t{int(e['from'])}\t+\t{int(e['to'])}\t+\t{G.k - 1}M" for e in G.edges]
    return out


def _fasta(G):
    out = []
    for i, (s, u) in enumerate(zip(G.strings(), G.unitigs)):
        out.append(f">u{i} nodes={int(u['nodes'])} kc={int(u['kmer_count'])}" + (" circular" if u["flags"] & CR.CIRCULAR else ""))
        out.append(s)
    return out


def _check(tmp_path, out, E, k, tag):
    G = CR.from_esa(E, k)
    r = _run("dbg", "-i", out, "-k", str(k))
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == _gfa(G)
    err = r.stderr.strip().splitlines()
    lens = [len(s) for s in G.strings()]
    assert len(err) == 1 and err[0].startswith("# dbg\t")
    for field in (f"k={k}", f"nodes={G.counts['nodes']}", f"unitigs={len(G.unitigs)}", f"edges={len(G.edges)}",
                  f"longest={max(lens, default=0)}", f"N50={CR.n50(lens)}", f"circular={G.counts['circular']}"):
        assert field in err[0].split("\t"), (field, err[0])
    r = _run("dbg", "-i", out, "-k", str(k), "--fasta")
    assert r.returncode == 0 and r.stdout.splitlines() == _fasta(G)
    # the k-mers of every S string, counted by the index, sum to its KC
    pat = tmp_path / f"{tag}_{k}.fa"
    names = []
    with open(pat, "w") as fh:
        for i, s in enumerate(G.strings()):
            for j in range(len(s) - k + 1):
                fh.write(f">{i}\n{s[j:j + k]}\n")
                names.append(i)
    r = _run("count", "-i", out, str(pat))
    assert r.returncode == 0, r.stderr
    sums = [0] * len(G.unitigs)
    rows = r.stdout.splitlines()
    assert len(rows) == len(names)
    for i, ln in zip(names, rows):
        name, c = ln.split("\t")[:2]
        assert int(name) == i and int(c) > 0
        sums[i] += int(c)
    assert sums == [int(u["kmer_count"]) for u in G.unitigs]
    return G


@pytest.mark.gpu
def test_dbg_of_a_builder_case(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    name = "dup_40x20"
    E, strs = ER.of_case(name), F.strings(F.geometry_cases()[name])
    out = _indexed(tmp_path, strs, "dup")
    G = _check(tmp_path, out, E, 8, "dup")
    assert len(G.unitigs) >= 1 and (G.unitigs["kmer_count"] % 20 == 0).all()
    _check(tmp_path, out, E, 3, "dup")
    r = _run("dbg", "-i", out, "-k", "41")                       # every record is shorter: an empty graph
    assert r.returncode == 0 and r.stdout.splitlines() == ["H\tVN:Z:1.0"] and "unitigs=0" in r.stderr


@pytest.mark.gpu
def test_dbg_of_the_pan_genome(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    recs = pan_genome()
    out = _indexed(tmp_path, F.strings(recs), "pan")
    G = _check(tmp_path, out, ER.Esa(recs), 21, "pan")
    assert (len(G.unitigs), len(G.edges)) == (487, 649)
