"""deBWT-query repeats (debwt_fm_repeats): option errors without a GPU; on the GPU, deBWT, index and repeats on a FASTA of
one builder case and of the seeded read set -- the header line and every repeat line against repeat_ref.py, the strings of
--seq against the records at every occurrence that --occurrences lists."""
import os
import subprocess

import pytest

import esa_ref as ER
import fm_definition as F
import kmer_ref as KR
import repeat_ref as RR
from conftest import ROOT

CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(*args):
    return subprocess.run([QUERY, *args], capture_output=True, text=True, timeout=300)


def test_repeats_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    o = str(tmp_path / "o")
    r = _run("repeats")                                          # -i is required
    assert r.returncode == 1 and "usage" in r.stderr and "deBWT-query repeats" in r.stderr
    r = _run("repeats", "-i", o, "reads.fa")                     # no file argument
    assert r.returncode == 1 and "usage" in r.stderr
    for opt, bad in (("--min-len", ("0", "x", "-3", "4294967296")), ("--min-occ", ("0", "1", "x", "-2")),
                     ("--max-occ", ("0", "1", "x")), ("--max-lcp", ("0", "x", "4294967296"))):
        for v in bad:
            r = _run("repeats", "-i", o, opt, v)
            assert r.returncode == 1 and opt in r.stderr and "usage" not in r.stderr, (opt, v)
    r = _run("repeats", "-i", o, "--min-occ", "5", "--max-occ", "4")
    assert r.returncode == 1 and "--max-occ" in r.stderr and "--min-occ" in r.stderr
    r = _run("repeats", "-i", o, "--supermaximal", "--intervals")
    assert r.returncode == 1 and "--supermaximal" in r.stderr and "usage" not in r.stderr
    r = _run("repeats", "-i", o, "--max-lcp", "20")              # the default --min-len is 20: nothing could be listed
    assert r.returncode == 1 and "--min-len" in r.stderr and "--max-lcp" in r.stderr
    for opt in ("--min-len", "--min-occ", "--max-occ", "--max-lcp"):
        r = _run("repeats", "-i", o, opt)                        # a value is missing
        assert r.returncode == 1 and "usage" in r.stderr
    for opt in (["--both-strands"], ["-k", "21"], ["--profile", "8"], ["--lcp", "l.bin"], ["--min-overlap", "20"], ["--all"]):
        r = _run("repeats", "-i", o, *opt)                       # the options of the others are none of repeats'
        assert r.returncode == 1 and "usage" in r.stderr, opt
    for cmd in ("lcp", "spectrum", "count", "extract", "graph"):  # and the options of repeats are none of theirs
        need = ["-k", "15"] if cmd == "spectrum" else []
        for opt in (["--min-occ", "3"], ["--max-occ", "3"], ["--supermaximal"], ["--intervals"], ["--seq"], ["--occurrences"]):
            r = _run(cmd, "-i", o, *need, *opt, *(["p.fa"] if cmd in ("count", "extract") else []))
            assert r.returncode == 1 and "usage" in r.stderr, (cmd, opt)
    r = _run("repeats", "-i", o)                                 # no such index: refused before anything is built
    assert r.returncode == 1 and r.stdout == ""


def _indexed(tmp_path, strs, tag):
    fa = tmp_path / f"{tag}.fa"
    fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(strs)))
    out = str(tmp_path / tag)
    r = subprocess.run([CLI, "-o", out, str(fa)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = _run("index", "-i", out, "--sa", "8", str(fa))
    assert r.returncode == 0, r.stderr
    return out


def _lines(E, rec):
    out = []
    for x in rec:
        a, b = E.resolve(int(E.sa[int(x["row_lo"])]))
        flag = "S" if x["flags"] & RR.IS_SUPERMAXIMAL else "M" if x["flags"] & RR.IS_MAXIMAL else "-"
        out.append(f"{x['len']}\t{x['count']}\t{flag}\t{','.join(str(int(v)) for v in x['left'])}\t{a}:{b}")
    return out


def _header(E, rec, min_len, max_lcp=0):
    every = RR.repeats(E, min_len=min_len, kind="intervals", max_lcp=max_lcp)
    return (f"# intervals={len(every)}\tmaximal={int((every['flags'] & RR.IS_MAXIMAL != 0).sum())}"
            f"\tsupermaximal={int((every['flags'] & RR.IS_SUPERMAXIMAL != 0).sum())}\treported={len(rec)}"
            f"\tlongest={int(rec['len'].max()) if len(rec) else 0}")


def _check(out, E, args, **kw):
    r = _run("repeats", "-i", out, *args)
    assert r.returncode == 0, r.stderr
    rec = RR.repeats(E, **kw)
    assert r.stdout.splitlines() == [_header(E, rec, kw.get("min_len", 20), kw.get("max_lcp", 0))] + _lines(E, rec), args
    assert len(r.stderr.strip().splitlines()) == 1 and r.stderr.startswith("repeats:")
    return rec


def _check_strings(out, E, strs, args, **kw):
    """--seq --occurrences: the string stands in the records at every listed occurrence, and the occurrences are the rows"""
    r = _run("repeats", "-i", out, "--seq", "--occurrences", *args)
    assert r.returncode == 0, r.stderr
    rec = RR.repeats(E, **kw)
    body = r.stdout.splitlines()[1:]
    assert [ln.rsplit("\t", 2)[0] for ln in body] == _lines(E, rec) and len(rec)
    for ln, x in zip(body, rec):
        seq, occ = ln.split("\t")[5:]
        places = [tuple(int(v) for v in o.split(":")) for o in occ.split(",")]
        assert len(seq) == x["len"] and len(places) == x["count"]
        assert places == [E.resolve(int(p)) for p in E.sa[int(x["row_lo"]):int(x["row_lo"] + x["count"])]]
        for j, off in places:
            assert strs[j][off:off + len(seq)] == seq


@pytest.mark.gpu
def test_repeats_of_a_builder_case(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    name = "dup_40x20"
    E, strs = ER.of_case(name), F.strings(F.geometry_cases()[name])
    out = _indexed(tmp_path, strs, "dup")
    rec = _check(out, E, ["--min-len", "1"], min_len=1)
    assert len(rec) > 5 and (rec["count"] >= 20).all()
    _check(out, E, ["--min-len", "40", "--intervals"], min_len=40, kind="intervals")
    _check(out, E, ["--min-len", "3", "--supermaximal", "--min-occ", "20", "--max-occ", "20"], min_len=3, kind="supermaximal",
           min_occ=20, max_occ=20)
    _check(out, E, ["--min-len", "2", "--max-lcp", "7", "--intervals"], min_len=2, kind="intervals", max_lcp=7)
    _check_strings(out, E, strs, ["--min-len", "30"], min_len=30)


@pytest.mark.gpu
def test_repeats_of_the_read_set(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    strs = KR.read_set()["records"]
    E = ER.of_read_set()
    out = _indexed(tmp_path, strs, "reads")
    rec = _check(out, E, [], min_len=20)
    assert len(rec) > 1000 and int(rec["len"].max()) == E.summary()["max"]
    _check(out, E, ["--supermaximal", "--min-len", "25"], min_len=25, kind="supermaximal")
    _check(out, E, ["--intervals", "--min-len", "12", "--min-occ", "5", "--max-occ", "10"], min_len=12, kind="intervals", min_occ=5,
           max_occ=10)
    _check_strings(out, E, strs, ["--min-len", "40", "--min-occ", "3"], min_len=40, min_occ=3)
