"""deBWT-query repeats --min-records / --max-records / --unique, mums and count --records (Definition 12): option errors
without a GPU; on the GPU, deBWT, index and the three commands on a FASTA of one builder case and of three mutated copies
of one genome -- every line against record_ref.py, and repeats without the new options as it was."""
import numpy as np
import pytest

import esa_ref as ER
import fm_definition as F
import record_ref as QR
import repeat_ref as RR
from test_cli_query_repeats import _have_query, _header, _indexed, _lines, _run


def test_records_option_errors(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    o = str(tmp_path / "o")
    r = _run("mums")                                             # -i is required
    assert r.returncode == 1 and "usage" in r.stderr and "deBWT-query mums" in r.stderr
    r = _run("mums", "-i", o, "reads.fa")                        # no file argument
    assert r.returncode == 1 and "usage" in r.stderr
    for cmd, opt in (("repeats", "--min-records"), ("repeats", "--max-records"), ("mums", "--min-records"), ("mums", "--min-len")):
        for v in ("0", "x", "-2"):
            r = _run(cmd, "-i", o, opt, v)
            assert r.returncode == 1 and opt in r.stderr and "usage" not in r.stderr, (cmd, opt, v)
        r = _run(cmd, "-i", o, opt)                              # a value is missing
        assert r.returncode == 1 and "usage" in r.stderr
    r = _run("repeats", "-i", o, "--min-records", "5", "--max-records", "4")
    assert r.returncode == 1 and "--max-records" in r.stderr and "--min-records" in r.stderr
    for opt in (["--max-records", "3"], ["--unique"], ["--min-occ", "3"], ["--intervals"], ["--occurrences"], ["--max-lcp", "30"]):
        r = _run("mums", "-i", o, *opt)                          # mums takes --min-len, --min-records and --seq alone
        assert r.returncode == 1 and "usage" in r.stderr, opt
    for cmd in ("lcp", "locate", "extract"):                     # and the new options are none of the others'
        for opt in (["--min-records", "3"], ["--unique"], ["--records"]):
            r = _run(cmd, "-i", o, *opt, *(["p.fa"] if cmd != "lcp" else []))
            assert r.returncode == 1 and "usage" in r.stderr, (cmd, opt)
    p = tmp_path / "p.fa"
    p.write_text(">a\nACGT\n")
    r = _run("count", "-i", o, "--records", "--both-strands", str(p))
    assert r.returncode == 1 and "--records" in r.stderr and r.stdout == ""
    r = _run("mums", "-i", o)                                    # no such index: refused before anything is built
    assert r.returncode == 1 and r.stdout == ""


def _rec_lines(E, rec, rc):
    out = []
    for ln, c in zip(_lines(E, rec), rc.tolist()):
        f = ln.split("\t")
        out.append("\t".join(f[:2] + [str(c)] + f[2:]))
    return out


def _check_records(out, E, args, **kw):
    r = _run("repeats", "-i", out, *args)
    assert r.returncode == 0, r.stderr
    rec, rc = QR.repeats(E, **kw)
    assert r.stdout.splitlines() == [_header(E, rec, kw.get("min_len", 20), kw.get("max_lcp", 0))] + _rec_lines(E, rec, rc), args
    return rec


def _check_mums(out, E, strs, args, **kw):
    r = _run("mums", "-i", out, "--seq", *args)
    assert r.returncode == 0, r.stderr
    rec, rc = QR.mums(E, **kw)
    q = kw.get("min_records") or len(E.records)
    lines = r.stdout.splitlines()
    assert lines[0] == f"# mums={len(rec)}\tmin_records={q}\tlongest={int(rec['len'].max()) if len(rec) else 0}"
    want = QR.mum_strings(E, rec)
    assert len(lines) - 1 == len(rec) == len(want)
    for ln, x in zip(lines[1:], rec):
        length, occ, seq = ln.split("\t")
        places = tuple(tuple(int(v) for v in o.split(":")) for o in occ.split(","))
        assert int(length) == x["len"] == len(seq) and want[seq] == places and len(places) == x["count"] >= q
        assert [j for j, _ in places] == sorted({j for j, _ in places})         # ascending, one per record
        for j, off in places:
            assert strs[j][off:off + len(seq)] == seq
    plain = _run("mums", "-i", out, *args)
    assert plain.returncode == 0 and plain.stdout.splitlines() == [ln.rsplit("\t", 1)[0] if i else ln for i, ln in enumerate(lines)]
    return rec


def _check_count(out, tmp_path, E, strs, rng):
    pats = []
    for s in strs:
        for _ in range(12):
            a = int(rng.integers(0, len(s) - 1))
            pats.append(s[a:a + int(rng.integers(1, 25))])
    pats += ["ACGTACGTTTGACA", "T", "GG"]
    fa = tmp_path / "pat.fa"
    fa.write_text("".join(f">p{i}\n{p}\n" for i, p in enumerate(pats)))
    r = _run("count", "-i", out, "--records", str(fa))
    assert r.returncode == 0, r.stderr
    want = [f"p{i}\t{sum(len(QR.occurrences(s, p)) for s in strs)}\t{sum(p in s for s in strs)}" for i, p in enumerate(pats)]
    assert r.stdout.splitlines() == want
    plain = _run("count", "-i", out, str(fa))                                   # without the option, as it was
    assert plain.returncode == 0 and plain.stdout.splitlines() == [w.rsplit("\t", 1)[0] for w in want]


@pytest.mark.gpu
def test_records_of_a_builder_case(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    name = "dup_40x20"
    E, strs = ER.of_case(name), F.strings(F.geometry_cases()[name])
    out = _indexed(tmp_path, strs, "dup")
    rec = _check_records(out, E, ["--min-len", "1", "--min-records", "1"], min_len=1)
    assert np.array_equal(rec, RR.repeats(E, min_len=1)) and len(rec) > 5
    _check_records(out, E, ["--min-len", "2", "--intervals", "--unique"], min_len=2, kind="intervals", unique=True)
    _check_records(out, E, ["--min-len", "2", "--intervals", "--max-records", "19", "--max-lcp", "7"], min_len=2, kind="intervals",
                   max_records=19, max_lcp=7)
    assert len(_check_mums(out, E, strs, ["--min-len", "1"], min_len=1)) >= 1
    _check_count(out, tmp_path, E, strs, np.random.default_rng(5))
    # repeats without the new options: the lines of test_cli_query_repeats, no column added
    r = _run("repeats", "-i", out, "--min-len", "1")
    want = RR.repeats(E, min_len=1)
    assert r.returncode == 0 and r.stdout.splitlines() == [_header(E, want, 1)] + _lines(E, want)


@pytest.mark.gpu
def test_mums_of_mutated_copies(tmp_path):
    assert _have_query(), "cli/deBWT-query is not built"
    recs = QR.mutated_copies(11)
    E, strs = ER.Esa(recs), F.strings(recs)
    out = _indexed(tmp_path, strs, "pan")
    rec = _check_mums(out, E, strs, ["--min-len", "5"], min_len=5)
    assert len(rec) >= 5 and QR.mum_strings(E, rec) == {w: o for w, o in QR.brute_mums(E, 5).items()}
    two = _check_mums(out, E, strs, ["--min-len", "8", "--min-records", "2"], min_len=8, min_records=2)
    assert len(two) > len(QR.mums(E, min_len=8)[0])
    _check_records(out, E, ["--min-len", "4", "--min-records", "2", "--max-records", "2"], min_len=4, min_records=2, max_records=2)
    _check_count(out, tmp_path, E, strs, np.random.default_rng(6))
