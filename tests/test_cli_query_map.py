"""deBWT-query map (debwt_fm_map): option errors without a GPU; on the GPU, index then map on a golden FASTA, every PAF
line against the Python API's result for the same reads, a wrong --ref refused, the other subcommands untouched."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(*args):
    return subprocess.run([QUERY, *args], capture_output=True, text=True, timeout=300)


def _revcomp(p):
    return "".join(COMP.get(c, "N") for c in reversed(p.upper()))


def test_map_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    fa = os.path.join(GOLDEN, "shared_ends_duplicates.fa")
    r = _run("map", "-i", str(tmp_path / "o"), "r.fa")                    # no --ref
    assert r.returncode == 1 and "--ref" in r.stderr and not r.stdout
    for opt, v in (("--band", "64"), ("--band", "x"), ("--max-occ", "0"), ("--min-score", "-3"), ("--min-len", "0")):
        r = _run("map", "-i", str(tmp_path / "o"), "--ref", fa, opt, v, "r.fa")
        assert r.returncode == 1 and opt in r.stderr, (opt, v)
    for opt in (["--both-strands"], ["--mismatches", "1"], ["--max-hits", "3"]):
        r = _run("map", "-i", str(tmp_path / "o"), "--ref", fa, *opt, "r.fa")
        assert r.returncode == 1 and "usage" in r.stderr
    for cmd in ("count", "mems"):
        r = _run(cmd, "-i", str(tmp_path / "o"), "--ref", fa, "r.fa")
        assert r.returncode == 1 and "usage" in r.stderr
    reads = tmp_path / "r.fa"
    reads.write_text(">a\nACGTACGTACGTACGTACGTACGT\n")
    r = _run("map", "-i", str(tmp_path / "missing"), "--ref", fa, str(reads))   # no OUT.sa
    assert r.returncode == 1 and ".sa" in r.stderr and not r.stdout
    r = _run("map", "--ref", fa, str(reads))
    assert r.returncode == 1 and "usage" in r.stderr and "map" in r.stderr


@pytest.mark.gpu
def test_map_end_to_end(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    from debwt_amd import api, fasta
    fa = os.path.join(GOLDEN, "shared_ends_duplicates.fa")
    codes = fasta.read_fasta(fa)[1]
    recs = ["".join("ACGT"[c] for c in r) for r in codes]
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, fa], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", fa)
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(8)
    reads = []
    for i in range(30):
        rec = recs[int(rng.integers(0, len(recs)))]
        L = int(rng.integers(40, 120))
        p = int(rng.integers(0, len(rec) - L))
        s = list(rec[p:p + L])
        for _ in range(int(rng.integers(0, 4))):
            j = int(rng.integers(1, len(s) - 1))
            kind = int(rng.integers(0, 3))
            if kind == 0:
                s[j] = "ACGTN"[int(rng.integers(0, 5))]
            elif kind == 1:
                s.insert(j, "ACGT"[int(rng.integers(0, 4))])
            else:
                del s[j]
        s = "".join(s)
        reads.append(_revcomp(s) if i % 2 else s)
    reads += ["N" * 30, "ACGTACGTAC", ""]
    pf = tmp_path / "r.fq"
    pf.write_text("".join(f"@r{i} x\n{p}\n+\n{'I' * len(p)}\n" for i, p in enumerate(reads)))
    d = api.DeBWT(k=32)
    d.load_records(codes)
    d.build()
    fm = d.fm_index(sa_sample=8)
    fm.attach_text(d)
    d.close()
    for opts, kw in (([], {}), (["--min-len", "12", "--band", "5", "--max-occ", "3", "--min-score", "20"],
                                dict(min_len=12, band=5, max_occ=3, min_score=20))):
        res = fm.map(reads, **kw)
        r = _run("map", "-i", out, "--ref", fa, *opts, str(pf))
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        mapped = [i for i in range(len(reads)) if res.mapped[i]]
        assert len(lines) == len(mapped) and len(mapped) >= 1
        for line, i in zip(lines, mapped):
            f = line.split("\t")
            m = len(reads[i])
            rev = bool(res.strand[i])
            qb, qe = int(res.qbeg[i]), int(res.qend[i])
            ops = [(int(x) >> 4, int(x) & 15) for x in res.ops(i)]
            cols = sum(n for n, _ in ops)
            gaps = sum(n for n, k in ops if k)
            match = cols - gaps - (int(res.edits[i]) - gaps)
            rec = int(res.record[i])
            want = [f"r{i}", str(m), str(m - qe if rev else qb), str(m - qb if rev else qe), "-" if rev else "+", str(rec),
                    str(len(recs[rec])), str(int(res.offset[i])), str(int(res.offset[i]) + int(res.tend[i]) - int(res.tbeg[i])),
                    str(match), str(cols), str(int(res.mapq[i])), f"AS:i:{int(res.score[i])}", f"NM:i:{int(res.edits[i])}",
                    f"cg:Z:{res.cigar(i)}"]
            assert f == want, (opts, line)
            # the PAF query interval is on the read as given: it reads (the reverse complement of) the target interval
            if int(res.edits[i]) == 0:
                t = recs[rec][int(f[7]):int(f[8])]
                assert reads[i][int(f[2]):int(f[3])].upper() == (_revcomp(t) if rev else t)
    fm.close()
    # not the text of OUT: another FASTA, and the same records with one boundary moved
    r = _run("map", "-i", out, "--ref", os.path.join(GOLDEN, "lowercase_3x2500.fa"), str(pf))
    assert r.returncode == 1 and "not the text" in r.stderr and not r.stdout
    joined = recs[0] + recs[1][:1]
    moved = tmp_path / "moved.fa"
    moved.write_text(f">a\n{joined}\n>b\n{recs[1][1:]}\n" + "".join(f">r{k}\n{s}\n" for k, s in enumerate(recs[2:])))
    r = _run("map", "-i", out, "--ref", str(moved), str(pf))
    assert r.returncode == 1 and "not the text" in r.stderr and "separator" in r.stderr
    # the other subcommands print what they printed
    r0 = _run("count", "-i", out, str(pf))
    assert r0.returncode == 0 and all(len(x.split("\t")) == 2 for x in r0.stdout.splitlines())
    r1 = _run("mems", "-i", out, str(pf))
    assert r1.returncode == 0 and all(len(x.split("\t")) == 6 for x in r1.stdout.splitlines())
