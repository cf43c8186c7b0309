"""deBWT-query pileup and consensus (debwt_fm_pileup, debwt_fm_pile_call, debwt_fm_consensus): option errors without a
GPU; on the GPU the TSV, the FASTA and the variants on the planted input of tests/test_fm_pileup_gpu.py against what the
Python API gives for the same reads, with --region, with --window 1000 (several tables per record), with --chain and
--mate, and map's own output unchanged beside them."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(*args):
    return subprocess.run([QUERY, *args], capture_output=True, text=True, timeout=300)


def test_pileup_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    fa = os.path.join(GOLDEN, "shared_ends_duplicates.fa")
    o = str(tmp_path / "o")
    for cmd in ("pileup", "consensus"):
        for opt, v in (("--min-mapq", "61"), ("--window", "0"), ("--min-permille", "1001"), ("--min-depth", "x"), ("--band", "64")):
            r = _run(cmd, "-i", o, "--ref", fa, opt, v, "r.fa")
            assert r.returncode == 1 and opt in r.stderr, (cmd, opt)
        r = _run(cmd, "--ref", fa, "r.fa")
        assert r.returncode == 1 and "usage" in r.stderr and "pileup" in r.stderr
    r = _run("pileup", "-i", o, "--ref", fa, "--variants", "v.tsv", "r.fa")          # only consensus writes variants
    assert r.returncode == 1 and "usage" in r.stderr
    r = _run("map", "-i", o, "--ref", fa, "--min-mapq", "3", "r.fa")                 # and map takes none of the new options
    assert r.returncode == 1 and "usage" in r.stderr


def _pileup_lines(counts, ref, starts, window):
    out, r = [], 0
    ends = list(starts[1:]) + [None]
    for k, c in enumerate(counts.tolist()):
        t = window[0] + k
        d = sum(c[:5])
        if not d:
            continue
        while ends[r] is not None and t >= ends[r]:
            r += 1
        out.append("\t".join(str(x) for x in [r, t - starts[r] + 1, "ACGTN"[ref[k]], d] + c[:7]))
    return out


def _variant_lines(variants, voted, starts):
    out = []
    for t, depth, count, ins, ref, call in variants:
        r = max(k for k, s in enumerate(starts) if s <= t)
        b = call & 15
        if b != ref:
            out.append("\t".join(str(x) for x in (r, t - starts[r] + 1, "ACGT"[ref], "-" if b == 4 else "ACGT"[b], depth, count)))
        if call & 0x10:
            out.append("\t".join(str(x) for x in (r, t - starts[r] + 1, "ACGT"[ref], "+" + voted[t][0], depth, voted[t][1])))
    return out


@pytest.mark.gpu
def test_pileup_and_consensus_end_to_end(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    from debwt_amd import api
    from test_fm_pileup_gpu import E2E_SEED, index_of, planted_case, var_tuples
    strs, copies, reads, planted = planted_case(E2E_SEED)
    fa = tmp_path / "ref.fa"
    fa.write_text("".join(f">rec{i}\n{s}\n" for i, s in enumerate(strs)))
    pf = tmp_path / "reads.fa"
    pf.write_text("".join(f">r{i}\n{p}\n" for i, p in enumerate(reads)))
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, str(fa)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", str(fa))
    assert r.returncode == 0, r.stderr
    base = ["-i", out, "--ref", str(fa)]
    map_before = _run("map", *base, str(pf))
    assert map_before.returncode == 0 and map_before.stdout.count("\n") > 2000

    fm = index_of(api, strs)
    starts = [int(x) for x in fm.record_starts()]
    mp = fm.map(reads)
    res = mp.pileup(fm, reads, min_mapq=20)
    counts = res.counts
    cr = res.call()
    voted = {t: (s, sup, d) for t, s, sup, d in cr.insertions()}
    want_tsv = _pileup_lines(counts, cr.ref.tolist(), starts, res.window)
    want_fa = "".join(f">{r}\n{s}\n" for r, s in cr.consensus())
    want_var = _variant_lines(var_tuples(cr.variants), voted, starts)
    assert len(want_var) == 6 + 1 + 3 + 2

    for extra in ([], ["--window", "1000"]):
        r = _run("pileup", *base, *extra, str(pf))
        assert r.returncode == 0, r.stderr
        assert r.stdout.splitlines() == want_tsv, extra
        vf = tmp_path / "v.tsv"
        r = _run("consensus", *base, *extra, "--variants", str(vf), str(pf))
        assert r.returncode == 0, r.stderr
        assert r.stdout == want_fa, extra
        assert vf.read_text().splitlines() == want_var, extra
    assert [s.upper() for s in want_fa.splitlines()[1::2]] == copies

    # a region: the same lines, cut; the region's header; a lower quality cut and other call knobs reach the library
    rec, beg, end = 1, 500, 1700
    win = (starts[rec] + beg, starts[rec] + end)
    r = _run("pileup", *base, "--region", f"{rec}:{beg}-{end}", "--window", "500", str(pf))
    assert r.returncode == 0, r.stderr
    sub = mp.pileup(fm, reads, min_mapq=20, window=win)
    scr = sub.call()
    assert r.stdout.splitlines() == _pileup_lines(sub.counts, scr.ref.tolist(), starts, win)
    assert np.array_equal(sub.counts, counts[win[0]:win[1]])
    r = _run("consensus", *base, "--region", f"{rec}:{beg}-{end}", "--window", "500", str(pf))
    assert r.returncode == 0, r.stderr
    assert r.stdout == f">{rec}:{beg}-{end}\n{dict(scr.consensus())[rec]}\n"
    r = _run("consensus", *base, "--region", "2", "--min-mapq", "0", "--min-depth", "30", "--min-permille", "1000", str(pf))
    assert r.returncode == 0, r.stderr
    all0 = mp.pileup(fm, reads, min_mapq=0, window=(starts[2], starts[2] + len(strs[2]))).call(30, 1000)
    assert r.stdout == f">2\n{dict(all0.consensus())[2]}\n"
    r = _run("pileup", *base, "--region", "3", str(pf))
    assert r.returncode == 1 and "--region" in r.stderr

    # --chain and --mate are accepted and pile the same reads up
    r = _run("pileup", *base, "--chain", str(pf))
    assert r.returncode == 0 and len(r.stdout.splitlines()) == len(want_tsv)
    half = len(reads) // 2
    m1, m2 = tmp_path / "m1.fa", tmp_path / "m2.fa"
    m1.write_text("".join(f">p{i}\n{p}\n" for i, p in enumerate(reads[0:2 * half:2])))
    m2.write_text("".join(f">p{i}\n{p}\n" for i, p in enumerate(reads[1:2 * half:2])))
    r = _run("consensus", *base, "--mate", str(m2), str(m1))
    assert r.returncode == 0 and r.stdout.count(">") == 3, r.stderr
    mpp = fm.map_pairs(reads[0:2 * half:2], reads[1:2 * half:2])
    inter = [x for pr in zip(reads[0:2 * half:2], reads[1:2 * half:2]) for x in pr]
    assert r.stdout == "".join(f">{k}\n{s}\n" for k, s in mpp.pileup(fm, inter, min_mapq=20).consensus())

    # map prints what it printed before any of this
    again = _run("map", *base, str(pf))
    assert again.returncode == 0 and again.stdout == map_before.stdout
    lines = map_before.stdout.splitlines()
    mapped = np.flatnonzero(mp.mapped)
    assert len(lines) == len(mapped)
    for ln, i in zip(lines[:50], mapped[:50]):
        f = ln.split("\t")
        assert f[0] == f"r{i}" and int(f[5]) == int(mp.record[i]) and int(f[7]) == int(mp.offset[i]) and f[-1] == "cg:Z:" + mp.cigar(i)
    fm.close()
