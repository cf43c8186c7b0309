"""deBWT-query bidbg (debwt_fm_cdbg_both): option errors without a GPU; on the GPU, deBWT, index and bidbg on a FASTA of a
small read set sampled from both strands -- every S and L line parsed back against bicdbg_ref.py and against the API, the
two strings of every L line overlapping in the stated orientations, --fasta against the same strings, the stderr line, and
dbg on the same index printing what it printed before there was a bidbg."""
import os
import subprocess

import numpy as np
import pytest

import bicdbg_ref as BR
import cdbg_ref as CR
import esa_ref as ER
import fm_definition as F
from conftest import ROOT
from test_cli_query_dbg import CLI, QUERY, _fasta, _gfa, _have_query, _indexed, _run


def test_bidbg_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    o = str(tmp_path / "o")
    r = _run("bidbg")                                            # -i is required
    assert r.returncode == 1 and "usage" in r.stderr and "deBWT-query bidbg" in r.stderr
    r = _run("bidbg", "-k", "21")
    assert r.returncode == 1 and "usage" in r.stderr
    r = _run("bidbg", "-i", o)                                   # -k is required
    assert r.returncode == 1 and "-k" in r.stderr
    r = _run("bidbg", "-i", o, "-k", "21", "reads.fa")           # no file argument
    assert r.returncode == 1 and "usage" in r.stderr
    for v in ("0", "x", "-3", "4294967295", "21x"):
        r = _run("bidbg", "-i", o, "-k", v)
        assert r.returncode == 1 and "-k" in r.stderr and "usage" not in r.stderr, v
    for v in ("2", "20", "4294967294"):                          # an even k: refused by name, before the index is looked for
        r = _run("bidbg", "-i", o, "-k", v)
        assert r.returncode == 1 and r.stderr.startswith("-k:") and "odd" in r.stderr and "usage" not in r.stderr, v
        assert "cannot read" not in r.stderr and r.stdout == ""
    for opt in (["--both-strands"], ["--min-len", "20"], ["--min-overlap", "20"], ["--max-lcp", "30"], ["--forward"], ["--seq"],
                ["--bins", "8"], ["--all-edges"], ["--clean"], ["--states", "s.txt"]):
        r = _run("bidbg", "-i", o, "-k", "21", *opt)             # the options of the others are none of bidbg's
        assert r.returncode == 1 and "usage" in r.stderr, opt
    r = _run("bidbg", "-i", o, "-k", "21", "--fasta")            # no such index: refused before anything is built
    assert r.returncode == 1 and r.stdout == "" and "usage" not in r.stderr


def small_reads():
    """120 reads of 40-60 bases from a random 600-base genome, every second one from the other strand, and one record
    that holds a 10-mer equal to its own reverse complement"""
    rng = np.random.default_rng(29)
    g = rng.integers(0, 4, 600).astype(np.uint8)
    recs = []
    for i in range(120):
        m = int(rng.integers(40, 61))
        a = int(rng.integers(0, 600 - m + 1))
        recs.append(BR.rc_codes(g[a:a + m]) if i & 1 else g[a:a + m].copy())
    hairpin = "TTGACCATGGTCAAGT" + "".join(F.ACGT[c] for c in rng.integers(0, 4, 30))       # GACCATGGTC is its own reverse complement
    recs.append(np.array([F.ACGT.index(c) for c in hairpin], dtype=np.uint8))
    return recs


def _parse(text, k):
    """(strings, KC, circular flags, edges as (2a + o, 2b + o)) of a GFA as bidbg writes it"""
    rows = text.splitlines()
    assert rows[0] == "H\tVN:Z:1.0"
    strs, kc, circ, edges = [], [], [], []
    for ln in rows[1:]:
        f = ln.split("\t")
        if f[0] == "S":
            assert not edges and int(f[1]) == len(strs) and f[3] == f"LN:i:{len(f[2])}" and f[4].startswith("KC:i:")
            assert f[5:] in ([], ["CL:Z:circular"])
            strs.append(f[2]); kc.append(int(f[4][5:])); circ.append(len(f) == 6)
        else:
            assert f[0] == "L" and len(f) == 6 and f[2] in "+-" and f[4] in "+-" and f[5] == f"{k - 1}M"
            edges.append((2 * int(f[1]) + (f[2] == "-"), 2 * int(f[3]) + (f[4] == "-")))
    return strs, kc, circ, edges


@pytest.mark.gpu
def test_bidbg_of_a_small_read_set(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    from debwt_amd import api
    from test_fm_esa_gpu import index_of
    recs = small_reads()
    E = ER.Esa(recs)
    out = _indexed(tmp_path, F.strings(recs), "reads")
    x = index_of(api, recs, 4)
    e = x.esa(sa=True, da=True)
    for k in (9, 15):
        G = BR.from_esa(E, k)
        A = e.cdbg(k, strands="both")
        r = _run("bidbg", "-i", out, "-k", str(k))
        assert r.returncode == 0, r.stderr
        strs, kc, circ, edges = _parse(r.stdout, k)
        assert strs == A.strings() == G.strings() and kc == A.unitigs["kmer_count"].tolist() == G.unitigs["kmer_count"].tolist()
        assert circ == [bool(f & CR.CIRCULAR) for f in A.unitigs["flags"]]
        assert edges == [(int(a), int(b)) for a, b in A.edges.tolist()] == [(int(a), int(b)) for a, b in G.edges.tolist()]
        if k == 9:
            assert len(edges) > 10 and any(a & 1 for a, _ in edges) and any(b & 1 for _, b in edges)
        for a, b in edges:                                       # the two strings overlap by k - 1 in the stated orientations
            sa = F.revcomp(strs[a >> 1]) if a & 1 else strs[a >> 1]
            sb = F.revcomp(strs[b >> 1]) if b & 1 else strs[b >> 1]
            assert sa[len(sa) - (k - 1):] == sb[:k - 1], (a, b)
        err = r.stderr.strip().splitlines()
        lens = [len(s) for s in strs]
        assert len(err) == 1 and err[0].startswith("# bidbg\t")
        for field in (f"k={k}", f"nodes={G.counts['nodes']}", f"unitigs={len(strs)}", f"circular={G.counts['circular']}",
                      f"edges={len(edges)}", f"hairpins={G.counts['hairpins']}", f"longest={max(lens)}", f"N50={CR.n50(lens)}"):
            assert field in err[0].split("\t"), (field, err[0])
        assert any(f.startswith("rounds=") for f in err[0].split("\t"))
        r = _run("bidbg", "-i", out, "-k", str(k), "--fasta")
        assert r.returncode == 0 and r.stdout.splitlines() == _fasta(G)
        # dbg on the same index prints Definition 13's graph in the form it always had
        F13 = CR.from_esa(E, k)
        r = _run("dbg", "-i", out, "-k", str(k))
        assert r.returncode == 0 and r.stdout.splitlines() == _gfa(F13) and r.stderr.startswith("# dbg\t")
        r = _run("dbg", "-i", out, "-k", str(k), "--fasta")
        assert r.returncode == 0 and r.stdout.splitlines() == _fasta(F13)
    assert BR.from_esa(E, 9).counts["hairpins"] >= 1
    x.close()
    r = _run("bidbg", "-i", out, "-k", "61")                     # every record is shorter: an empty graph
    assert r.returncode == 0 and r.stdout.splitlines() == ["H\tVN:Z:1.0"] and "unitigs=0" in r.stderr
