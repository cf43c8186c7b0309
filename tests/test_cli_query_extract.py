"""deBWT-query extract and map without --ref (debwt_fm_extract, debwt_fm_restore_text): after index, the FASTA comes back
from OUT, OUT.#, OUT.$ and OUT.sa alone, regions are cut as locate's coordinates say, a rebuilt BWT of the extracted
FASTA is the original byte for byte, and map prints the same PAF with and without --ref."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")
NAMES = ["lowercase_3x2500", "t1_three_records"]


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(*args):
    return subprocess.run([QUERY, *args], capture_output=True, text=True, timeout=300)


def _records(name):
    from debwt_amd import fasta
    return ["".join("ACGT"[c] for c in r) for r in fasta.read_fasta(os.path.join(GOLDEN, name + ".fa"))[1]]


def _parse(text):
    lines = text.splitlines()
    assert len(lines) % 2 == 0 and all(h.startswith(">") for h in lines[0::2])
    return [h[1:] for h in lines[0::2]], lines[1::2]


def test_extract_usage_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    o = str(tmp_path / "o")
    for args in (["extract", "-i", o], ["extract", "-i", o, "--all", "r.txt"], ["extract", "--all"],
                 ["extract", "-i", o, "--ref", "x.fa", "--all"], ["count", "-i", o, "--all", "p.fa"]):
        r = _run(*args)
        assert r.returncode == 1 and "usage" in r.stderr and "extract" in r.stderr and not r.stdout, args
    r = _run("extract", "-i", o, str(tmp_path / "none.txt"))
    assert r.returncode == 1 and "none.txt" in r.stderr and not r.stdout
    r = _run("extract", "-i", str(tmp_path / "missing"), "--all")           # no OUT.sa
    assert r.returncode == 1 and ".sa" in r.stderr and not r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_extract_end_to_end(tmp_path, name):
    assert _have_query(), "cli/deBWT-query is not built"
    fa = os.path.join(GOLDEN, name + ".fa")
    recs = _records(name)
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, "-k", "32", fa], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    # --all, the same from samples every row and every 1024 rows
    texts = []
    for s in ("1", "1024"):
        r = _run("index", "-i", out, "--sa", s, fa)
        assert r.returncode == 0, r.stderr
        r = _run("extract", "-i", out, "--all")
        assert r.returncode == 0, r.stderr
        texts.append(r.stdout)
    assert texts[0] == texts[1]
    names, seqs = _parse(texts[0])
    assert names == [str(j) for j in range(len(recs))] and seqs == recs
    # regions
    last = len(recs) - 1
    L = len(recs[last])
    regions = ["1", "0:0-1", f"{last}:{L - 40}-{L}", "2:5-5", f"{last}:17-230", "0"]
    rf = tmp_path / "regions.txt"
    rf.write_text("".join(x + "\n" for x in regions) + "\n")
    r = _run("extract", "-i", out, str(rf))
    assert r.returncode == 0, r.stderr
    names, seqs = _parse(r.stdout)
    assert names == regions
    assert seqs == [recs[1], recs[0][:1], recs[last][L - 40:], "", recs[last][17:230], recs[0]]
    for bad, word in (("0:0-999999", "0:0-999999"), ("x", "x"), ("0:5-3", "0:5-3"), (f"{len(recs)}", f"'{len(recs)}'"),
                      ("0:1", "0:1"), ("0:-1-4", "0:-1-4")):
        bf = tmp_path / "bad.txt"
        bf.write_text(f"0:0-10\n{bad}\n")
        r = _run("extract", "-i", out, str(bf))
        assert r.returncode == 1 and "bad.txt:2" in r.stderr and word in r.stderr and not r.stdout, (bad, r.stderr)
    # the extracted FASTA has the BWT it was extracted from
    back = tmp_path / "back.fa"
    back.write_text(texts[0])
    out2 = str(tmp_path / "out2")
    r = subprocess.run([CLI, "-o", out2, "-k", "32", str(back)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for suffix in ("", ".#", ".$"):
        assert open(out2 + suffix, "rb").read() == open(out + suffix, "rb").read(), suffix


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_map_without_ref_prints_the_paf_of_map_with_ref(tmp_path, name):
    assert _have_query(), "cli/deBWT-query is not built"
    fa = os.path.join(GOLDEN, name + ".fa")
    recs = _records(name)
    out = str(tmp_path / "out")
    r = subprocess.run([CLI, "-o", out, "-k", "32", fa], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "16", fa)
    assert r.returncode == 0, r.stderr
    comp = str.maketrans("ACGT", "TGCA")
    rng = np.random.default_rng(12)
    reads = []
    for i in range(300):
        rec = recs[int(rng.integers(0, len(recs)))]
        n = int(rng.integers(40, 130))
        p = int(rng.integers(0, len(rec) - n))
        s = list(rec[p:p + n])
        for _ in range(int(rng.integers(0, 3))):
            s[int(rng.integers(1, n - 1))] = "ACGT"[int(rng.integers(0, 4))]
        s = "".join(s)
        reads.append(s.translate(comp)[::-1] if i % 2 else s)
    pf = tmp_path / "reads.fa"
    pf.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(reads)))
    with_ref = _run("map", "-i", out, "--ref", fa, str(pf))
    assert with_ref.returncode == 0, with_ref.stderr
    without = _run("map", "-i", out, str(pf))
    assert without.returncode == 0, without.stderr
    assert without.stdout == with_ref.stdout and len(with_ref.stdout.splitlines()) >= 150
    half = reads[:150]
    m1, m2 = tmp_path / "m1.fa", tmp_path / "m2.fa"
    m1.write_text("".join(f">p{i}\n{s}\n" for i, s in enumerate(half)))
    m2.write_text("".join(f">p{i}\n{s}\n" for i, s in enumerate(reads[150:])))
    a = _run("map", "-i", out, "--ref", fa, "--mate", str(m2), "--insert", "1,16000", str(m1))
    b = _run("map", "-i", out, "--mate", str(m2), "--insert", "1,16000", str(m1))
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout
