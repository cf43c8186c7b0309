"""deBWT-query map --chain (debwt_fm_map_chained): option parsing and the usage text without a GPU; on the GPU, index then
map --chain on a golden FASTA, every PAF line against FMIndex.map_chained for the same reads, and map without --chain
printing what FMIndex.map gives."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from test_cli_query_map import CLI, _have_query, _revcomp, _run


def test_chain_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    fa = os.path.join(GOLDEN, "shared_ends_duplicates.fa")
    base = ["map", "-i", str(tmp_path / "o"), "--ref", fa]
    r = _run("map")
    assert r.returncode == 1 and "--chain [--max-gap G]" in r.stderr and "chains the seeds" in r.stderr
    for v in ("x", "-1", "4294967296"):
        r = _run(*base, "--chain", "--max-gap", v, "r.fa")
        assert r.returncode == 1 and "--max-gap" in r.stderr and "usage" not in r.stderr, v
    r = _run(*base, "--max-gap", "100", "r.fa")                           # --max-gap belongs to --chain
    assert r.returncode == 1 and "--max-gap" in r.stderr and "--chain" in r.stderr and not r.stdout
    r = _run(*base, "r.fa", "--chain", "--max-gap")                       # a value is missing
    assert r.returncode == 1 and "usage" in r.stderr
    for cmd in ("count", "locate", "mems", "index"):                      # the option belongs to map alone
        r = _run(cmd, "-i", str(tmp_path / "o"), "--chain", "r.fa")
        assert r.returncode == 1 and "usage" in r.stderr, cmd
    reads = tmp_path / "r.fa"
    reads.write_text(">a\nACGTACGTACGTACGTACGTACGT\n")
    r = _run("map", "-i", str(tmp_path / "missing"), "--ref", fa, "--chain", "--max-gap", "0", str(reads))   # parsed: no OUT.sa
    assert r.returncode == 1 and ".sa" in r.stderr and not r.stdout


@pytest.mark.gpu
def test_map_chain_end_to_end(tmp_path):
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
    rng = np.random.default_rng(9)
    reads = []
    for i in range(30):
        rec = recs[int(rng.integers(0, len(recs)))]
        L = int(rng.integers(60, min(len(rec), 300)))
        p = int(rng.integers(0, len(rec) - L))
        s = list(rec[p:p + L])
        for _ in range(int(rng.integers(0, 4))):                          # substitutions, and indels of up to 8 bases
            j = int(rng.integers(1, len(s) - 9))
            kind = int(rng.integers(0, 3))
            n = int(rng.integers(1, 9))
            if kind == 0:
                s[j] = "ACGTN"[int(rng.integers(0, 5))]
            elif kind == 1:
                s[j:j] = ["ACGT"[int(x)] for x in rng.integers(0, 4, n)]
            else:
                del s[j:j + n]
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

    def paf(res):
        lines = []
        for i in range(len(reads)):
            if not res.mapped[i]:
                continue
            m, rev = len(reads[i]), bool(res.strand[i])
            qb, qe = int(res.qbeg[i]), int(res.qend[i])
            ops = [(int(x) >> 4, int(x) & 15) for x in res.ops(i)]
            cols = sum(n for n, _ in ops)
            gaps = sum(n for n, k in ops if k)
            match = cols - gaps - (int(res.edits[i]) - gaps)
            rec = int(res.record[i])
            lines.append("\t".join([
                f"r{i}", str(m), str(m - qe if rev else qb), str(m - qb if rev else qe), "-" if rev else "+", str(rec),
                str(len(recs[rec])), str(int(res.offset[i])), str(int(res.offset[i]) + int(res.tend[i]) - int(res.tbeg[i])),
                str(match), str(cols), str(int(res.mapq[i])), f"AS:i:{int(res.score[i])}", f"NM:i:{int(res.edits[i])}",
                f"cg:Z:{res.cigar(i)}"]))
        return lines

    for opts, kw in ((["--chain"], {}),
                     (["--chain", "--max-gap", "30", "--min-len", "12", "--band", "5", "--max-occ", "3", "--min-score", "20"],
                      dict(max_gap=30, min_len=12, band=5, max_occ=3, min_score=20))):
        want = paf(fm.map_chained(reads, **kw))
        r = _run("map", "-i", out, "--ref", fa, *opts, str(pf))
        assert r.returncode == 0, r.stderr
        assert len(want) >= 10 and r.stdout.splitlines() == want, opts
    # without --chain: what map printed before, i.e. FMIndex.map
    r = _run("map", "-i", out, "--ref", fa, str(pf))
    assert r.returncode == 0 and r.stdout.splitlines() == paf(fm.map(reads))
    fm.close()
