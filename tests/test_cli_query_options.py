"""deBWT-query: which subcommand takes which option, and which values each numeric option takes -- all 18 x 60 cells of
the command line, probed without an index and without a GPU: every probe is a process that ends in main() or, for a flag
or a file name that is accepted, at the first file that does not exist.

`python tests/test_cli_query_options.py BINARY` prints one line per probe (arguments, exit status, stderr) as JSON: the
transcripts of two builds are compared with diff."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli", "deBWT")
QUERY = os.path.join(ROOT, "cli", "deBWT-query")

# the contract, written out by hand: the options of every subcommand beside -i and --device, which all of them take
MAP = "--ref -t --iupac --min-len --band --max-occ --min-score --chain --max-gap --mate --insert --no-rescue"
PILEUP = MAP + " --min-mapq --region --window --min-depth --min-permille"
UNITIGS = "--min-overlap --both-strands --states --clean --max-tip --max-bubble --clean-rounds"
TABLE = {
    "index": "-t --iupac --sa",
    "count": "--mismatches --both-strands --best --records",
    "locate": "--max-hits --mismatches --both-strands --best",
    "mems": "--min-len --both-strands --max-hits",
    "map": MAP,
    "pileup": PILEUP,
    "consensus": PILEUP + " --variants",
    "overlaps": "--min-overlap --both-strands --longest --no-self --max-mismatches --max-error-permille",
    "extract": "--all",
    "kmers": "-k --both-strands",
    "correct": "-k --min-count --rounds --forward --report",
    "spectrum": "-k --forward --bins --list --at-least --at-most",
    "lcp": "--max-lcp --lcp --sa --da --profile",
    "repeats": "--min-len --min-occ --max-occ --supermaximal --intervals --max-lcp --seq --occurrences --min-records "
               "--max-records --unique",
    "mums": "--min-len --min-records --seq",
    "dbg": "-k --fasta",
    "graph": UNITIGS + " --all-edges",
    "unitigs": UNITIGS,
}
TABLE = {c: ["-i", "--device"] + o.split() for c, o in TABLE.items()}
COMMANDS = list(TABLE)

OPTIONS = ("-i --device -t --iupac --sa --mismatches --both-strands --best --records --max-hits --min-len --ref --band "
           "--max-occ --min-score --chain --max-gap --mate --insert --no-rescue --min-mapq --region --window --min-depth "
           "--min-permille --variants --min-overlap --longest --no-self --max-mismatches --max-error-permille --all -k "
           "--min-count --rounds --forward --report --bins --list --at-least --at-most --max-lcp --lcp --da --profile "
           "--min-occ --supermaximal --intervals --seq --occurrences --min-records --max-records --unique --fasta "
           "--all-edges --states --clean --max-tip --max-bubble --clean-rounds").split()
FLAGS = set("--both-strands --best --records --chain --no-rescue --longest --no-self --all --forward --supermaximal "
            "--intervals --seq --occurrences --unique --fasta --all-edges --clean".split())
STRINGS = set("-i --ref --mate --region --variants --report --list --lcp --da --states".split())   # and --sa of lcp
MAPPING = ("map", "pileup", "consensus")
ONLY_WITH_MAP = ("--mate", "--insert", "--no-rescue")
NEED_K = ("kmers", "correct", "spectrum", "dbg")
NO_FILE = ("spectrum", "lcp", "repeats", "mums", "dbg", "graph", "unitigs")

VALUES = ["", "x", "-1", "0", "1", "2", "3", "4", "5", "8", "12", "16", "17", "31", "32", "33", "60", "61", "63", "64",
          "255", "256", "257", "1000", "1001", "1024", "1025", "2048", "4096", "4097", "65535", "65536", "2147483647",
          "2147483648", "4294967294", "4294967295", "4294967296", "4294967297", "18446744073709551615", "1,2", "2,1", "auto"]

# the values of VALUES that a numeric option takes, per option and group of commands: the numbers from lo to hi and the
# words named behind them, or, in a row of one string, those values alone.  Recorded from the binary of the commit before
# the option table, not from the table
M32, M64 = 2**32 - 1, 2**64 - 1
TAKEN = [
    ("--device", " ".join(COMMANDS), 0, 255),
    ("-t", "index map pileup consensus", 1, M64),
    ("--iupac", "index map pileup consensus", 0, M64),
    ("--sa", "index", "1 2 4 8 16 32 64 256 1024"),
    ("--mismatches", "count locate", 0, 4),
    ("--max-hits", "locate mems", 0, M64),
    ("--min-len", "mems map pileup consensus repeats mums", 1, M32),
    ("--band", "map pileup consensus", 0, 63),
    ("--max-occ", "map pileup consensus", 1, M32),
    ("--max-occ", "repeats", 2, M64),
    ("--min-score", "map pileup consensus", 0, 2**31 - 1),
    ("--max-gap", "map pileup consensus", 0, M32),
    ("--insert", "map pileup consensus", "1,2"),
    ("--min-mapq", "pileup consensus", 0, 60),
    ("--window", "pileup consensus", 1, 2**32),
    ("--min-depth", "pileup consensus", 0, M32),
    ("--min-permille", "pileup consensus", 0, 1000),
    ("--min-overlap", "overlaps graph unitigs", 1, M32),
    ("--max-mismatches", "overlaps", 0, 4),
    ("--max-error-permille", "overlaps", 0, 1000),
    ("-k", "kmers correct", 1, M32),
    ("-k", "spectrum", 1, 32),
    ("-k", "dbg", 1, M32 - 1),
    ("--min-count", "correct", 1, M32, "auto"),
    ("--rounds", "correct", 1, 16),
    ("--bins", "spectrum", 2, 4096),
    ("--at-least", "spectrum", 1, M32),
    ("--at-most", "spectrum", 1, M32),
    ("--max-lcp", "lcp repeats", 1, M32),
    ("--profile", "lcp", 1, 4096),
    ("--min-occ", "repeats", 2, M64),
    ("--min-records", "repeats mums", 1, M64),
    ("--max-records", "repeats", 1, M64),
    ("--max-tip", "graph unitigs", 0, M32),
    ("--max-bubble", "graph unitigs", 0, M32),
    ("--clean-rounds", "graph unitigs", 1, M32),
]


def _values(lo, hi=None, words=""):
    if hi is None:
        return set(lo.split())
    return {v for v in VALUES if v.isdigit() and lo <= int(v) <= hi} | set(words.split())


TAKEN = {(o, c): _values(*r) for o, cs, *r in TAKEN for c in cs.split()}


def _have_query():
    if not (os.path.exists(QUERY) and os.path.exists(CLI)):
        subprocess.call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.exists(QUERY) and os.path.exists(CLI)


def _run(binary, args):
    r = subprocess.run([binary, *args], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr


def _numeric(cmd, opt):
    return opt not in FLAGS and opt not in STRINGS and (cmd, opt) != ("lcp", "--sa")


def _bare(cmd, opt):
    """CMD OPT [x], without -i: a numeric option that the command takes reports `OPT: ...`, everything else ends in the
    usage text or in `OPT: only with map`"""
    return [cmd, opt] + ([] if opt in FLAGS else ["x"])


def _full(cmd, opt):
    """CMD -i /nonexistent/o [-k 15] OPT [x] [FILE]: a flag or a file name that the command takes gets as far as the first
    file that is not there"""
    args = [cmd, "-i", "/nonexistent/o"] + (["-k", "15"] if cmd in NEED_K else []) + _bare(cmd, opt)[1:]
    return args + ([] if cmd in NO_FILE or (cmd, opt) == ("extract", "--all") else ["/nonexistent/f.fa"])


def _took(opt, err):
    return err.startswith(opt + ":") and "only with map" not in err


def test_the_contract_is_whole():
    assert len(COMMANDS) == 18 and len(OPTIONS) == 60 == len(set(OPTIONS))
    assert all(set(o) <= set(OPTIONS) and len(o) == len(set(o)) for o in TABLE.values())
    assert sum(len(o) for o in TABLE.values()) == 153
    numeric = {(o, c) for c in COMMANDS for o in TABLE[c] if _numeric(c, o)}
    assert set(TAKEN) == numeric and all(v <= set(VALUES) for v in TAKEN.values())


def test_option_names_of_the_table():
    """every name in front of a row of the option table of query.c is one of the 60, and the other way round"""
    src = open(os.path.join(ROOT, "cli", "query.c")).read()
    assert set(re.findall(r'^ {4}\{"(--?[a-z][a-z-]*)", ', src, re.M)) == set(OPTIONS)


@pytest.mark.parametrize("cmd", COMMANDS)
def test_which_options_a_command_takes(cmd):
    assert _have_query(), "cli/deBWT-query is not built"
    for opt in OPTIONS:
        rc, err = _run(QUERY, _bare(cmd, opt))
        assert rc == 1, (cmd, opt, rc, err[:200])
        if opt in TABLE[cmd]:
            if _numeric(cmd, opt):
                assert _took(opt, err), (cmd, opt, err[:200])
                continue
            assert err.startswith("usage:") or opt == "-i", (cmd, opt, err[:200])      # -i is missing, nothing else
            if cmd == "index":
                continue                                                     # -i: the next stop would be the GPU
            rc, err = _run(QUERY, _full(cmd, opt))
            assert rc == 1 and not err.startswith("usage:") and "only with map" not in err, (cmd, opt, rc, err[:200])
            continue
        for args in (None, _full(cmd, opt)):
            if args:
                rc, err = _run(QUERY, args)
            if opt in ONLY_WITH_MAP and cmd not in MAPPING:
                assert (rc, err) == (1, opt + ": only with map\n"), (cmd, opt, args, rc, err[:200])
            else:
                assert rc == 1 and err.startswith("usage:"), (cmd, opt, args, rc, err[:200])


@pytest.mark.parametrize("cmd", COMMANDS)
def test_which_values_a_numeric_option_takes(cmd):
    assert _have_query(), "cli/deBWT-query is not built"
    for opt in TABLE[cmd]:
        if not _numeric(cmd, opt):
            continue
        taken = set()
        for v in VALUES:
            rc, err = _run(QUERY, [cmd, opt, v])
            assert rc == 1 and (err.startswith("usage:") or _took(opt, err)), (cmd, opt, v, rc, err[:200])
            if err.startswith("usage:"):
                taken.add(v)
        assert taken == TAKEN[opt, cmd], (cmd, opt, sorted(taken ^ TAKEN[opt, cmd]))


def transcript(binary, out=sys.stdout):
    """every probe of the two tests above, and the values of every numeric option that this binary takes, cell by cell"""
    def probe(args):
        rc, err = _run(binary, args)
        out.write(json.dumps([args, rc, err]) + "\n")
        return err
    for cmd in COMMANDS:
        for opt in OPTIONS:
            err = probe(_bare(cmd, opt))
            if _took(opt, err):
                for v in VALUES:
                    probe([cmd, opt, v])
            elif not (cmd == "index" and opt in TABLE[cmd]):
                probe(_full(cmd, opt))


if __name__ == "__main__":
    transcript(sys.argv[1])
