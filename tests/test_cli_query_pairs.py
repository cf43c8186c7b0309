"""deBWT-query map --mate (debwt_fm_map_pairs): option errors without a GPU, the existing map invocations as they were; on
the GPU, index then map pairs cut from a golden FASTA, every PAF line and tag against FMIndex.map_pairs for the same reads."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from test_cli_query_map import CLI, _have_query, _revcomp, _run


def test_pair_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    fa = os.path.join(GOLDEN, "lowercase_3x2500.fa")
    o = str(tmp_path / "o")
    base = ["map", "-i", o, "--ref", fa]
    for args, opt in ((["--mate", "m.fa", "--chain"], "--mate"), (["--chain", "--mate", "m.fa"], "--mate"),
                      (["--mate", "m.fa", "--insert", "5"], "--insert"), (["--mate", "m.fa", "--insert", "500,200"], "--insert"),
                      (["--mate", "m.fa", "--insert", "a,b"], "--insert"), (["--mate", "m.fa", "--insert", "1,20000"], "--insert"),
                      (["--mate", "m.fa", "--insert", "0,0"], "--insert"), (["--insert", "200,500"], "--insert"),
                      (["--no-rescue"], "--no-rescue")):
        r = _run(*base, *args, "r.fa")
        assert r.returncode == 1 and opt in r.stderr and "usage" not in r.stderr and not r.stdout, (args, r.stderr)
    for cmd in ("count", "locate", "mems"):
        for args, opt in ((["--mate", "m.fa"], "--mate"), (["--no-rescue"], "--no-rescue"), (["--insert", "1,2"], "--insert")):
            r = _run(cmd, "-i", o, *args, "r.fa")
            assert r.returncode == 1 and opt in r.stderr and not r.stdout, (cmd, args)
    # the map invocations that exist behave as before: a second positional file is a usage error, not a mate
    r = _run(*base, "r.fa", "m.fa")
    assert r.returncode == 1 and "usage" in r.stderr
    r = _run("map", "-i", o, "r.fa")
    assert r.returncode == 1 and "--ref" in r.stderr
    r = _run(*base, "--max-gap", "10", "r.fa")
    assert r.returncode == 1 and "--max-gap" in r.stderr
    reads = tmp_path / "r.fa"
    reads.write_text(">a\nACGTACGTACGTACGTACGTACGT\n")
    r = _run("map", "-i", str(tmp_path / "missing"), "--ref", fa, str(reads))
    assert r.returncode == 1 and ".sa" in r.stderr and not r.stdout
    r = _run("map", "-i", str(tmp_path / "missing"), "--ref", fa, "--mate", str(tmp_path / "none.fa"), str(reads))
    assert r.returncode == 1 and "none.fa" in r.stderr and not r.stdout


def paf_of(res, names, reads, recs, i):
    m = len(reads[i])
    rev = bool(res.strand[i])
    qb, qe = int(res.qbeg[i]), int(res.qend[i])
    ops = [(int(x) >> 4, int(x) & 15) for x in res.ops(i)]
    cols = sum(n for n, _ in ops)
    gaps = sum(n for n, k in ops if k)
    match = cols - gaps - (int(res.edits[i]) - gaps)
    rec = int(res.record[i])
    want = [names[i], str(m), str(m - qe if rev else qb), str(m - qb if rev else qe), "-" if rev else "+", str(rec),
            str(len(recs[rec])), str(int(res.offset[i])), str(int(res.offset[i]) + int(res.tend[i]) - int(res.tbeg[i])),
            str(match), str(cols), str(int(res.mapq[i])), f"AS:i:{int(res.score[i])}", f"NM:i:{int(res.edits[i])}",
            f"cg:Z:{res.cigar(i)}"]
    proper = bool(int(res.flags[i]) & 8)
    want.append("pr:A:P" if proper else "pr:A:U")
    if proper:
        t = int(res.pairs["tlen"][i // 2])
        want.append(f"tl:i:{-t if rev else t}")
    if int(res.flags[i]) & 16:
        want.append("rs:i:1")
    return want


@pytest.mark.gpu
def test_map_pairs_end_to_end(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    from debwt_amd import api, fasta
    fa = os.path.join(GOLDEN, "lowercase_3x2500.fa")
    codes = fasta.read_fasta(fa)[1]
    recs = ["".join("ACGT"[c] for c in r) for r in codes]
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, fa], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", fa)
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(31)
    r1, r2 = [], []
    for p in range(45):
        rec = recs[p % len(recs)]
        T = int(rng.integers(200, 301))
        f = int(rng.integers(0, len(rec) - T))
        fw, rv = rec[f:f + 80], _revcomp(rec[f + T - 80:f + T])
        if p % 5 == 4:                                     # a mate without a seed: a substitution at every 16th base
            s = list(rv)
            for j in range(p % 16, len(s), 16):
                s[j] = "ACGT"[("ACGT".index(s[j]) + 1 + p % 3) % 4]
            rv = "".join(s)
        if p % 2:
            fw, rv = rv, fw
        r1.append(fw)
        r2.append(rv)
    r1.append("N" * 40)                                    # a pair that does not map at all
    r2.append("ACGTACGTAC")
    f1, f2 = tmp_path / "r1.fq", tmp_path / "r2.fa"
    f1.write_text("".join(f"@p{i}/1 x\n{p}\n+\n{'I' * len(p)}\n" for i, p in enumerate(r1)))
    f2.write_text("".join(f">p{i}/2\n{p}\n" for i, p in enumerate(r2)))
    names = [n for i in range(len(r1)) for n in (f"p{i}/1", f"p{i}/2")]
    reads = [r for pr in zip(r1, r2) for r in pr]
    d = api.DeBWT(k=32)
    d.load_records(codes)
    d.build()
    fm = d.fm_index(sa_sample=8)
    fm.attach_text(d)
    d.close()
    seen = set()
    # the three records are copies of one another but for a few bases: no pair maps uniquely, so the bounds cannot be estimated
    r = _run("map", "-i", out, "--ref", fa, "--mate", str(f2), str(f1))
    assert r.returncode == 1 and "insert bounds" in r.stderr and not r.stdout
    for opts, kw in ((["--insert", "100,600"], dict(insert=(100, 600))), (["--insert", "150,400"], dict(insert=(150, 400))),
                     (["--insert", "150,400", "--no-rescue", "--min-score", "25"], dict(insert=(150, 400), max_rescue=0, min_score=25))):
        res = fm.map_pairs(r1, r2, **kw)
        r = _run("map", "-i", out, "--ref", fa, "--mate", str(f2), *opts, str(f1))
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        mapped = [i for i in range(len(reads)) if res.mapped[i]]
        assert len(lines) == len(mapped) and len(mapped) >= 2 * 45 - 9
        for line, i in zip(lines, mapped):
            assert line.split("\t") == paf_of(res, names, reads, recs, i), (opts, line)
            seen.update(t[:6] if t.startswith("tl:i:-") else t[:5] if t.startswith("tl") else t for t in line.split("\t")[15:])
    assert seen == {"pr:A:P", "pr:A:U", "tl:i:", "tl:i:-", "rs:i:1"}
    fm.close()
    short = tmp_path / "short.fa"
    short.write_text("".join(f">p{i}/2\n{p}\n" for i, p in enumerate(r2[:-1])))
    r = _run("map", "-i", out, "--ref", fa, "--mate", str(short), str(f1))
    assert r.returncode == 1 and "--mate" in r.stderr and not r.stdout
