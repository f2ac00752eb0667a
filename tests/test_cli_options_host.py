"""The command lines of the seven commands (bam2db, crb, extract, freq, filter, and sweep / cap / level), without a device: every
run here ends in a parse error, in the help text or in one of the checks behind the option loop, and every case pins the exact
(exit status, stdout, stderr).  Two dialects are pinned: bam2db, crb, extract and the grid verbs stop at the first argument that
is no option and take no clusters; freq and filter skip such arguments and cluster their short options."""
import hashlib
import subprocess

import pytest

from fastf_amd import _lib

RED = "\x1b[31mError:\x1b[0m "
GRID = ("sweep", "cap", "level")
STOP = ("bam2db", "crb", "extract") + GRID
ARGPARSE = ("freq", "filter")
ALL = STOP + ARGPARSE
HUGE = "99999999999999999999"

# where the help text goes behind `unknown option`: bam2db and the grid verbs on stderr, freq and filter on stdout, crb and extract nowhere
USAGE = {"bam2db": "stderr", "sweep": "stderr", "cap": "stderr", "level": "stderr", "freq": "stdout", "filter": "stdout", "crb": None, "extract": None}
# the list of a grid verb, which cap and level miss before they look for an input file
LIST = {"sweep": [], "cap": ["-n", "3"], "level": ["-m", "2"], "bam2db": [], "crb": [], "extract": []}
# (long, short) of the options that take an integer, a float, and of one that takes any value
INTS = {"bam2db": [("seed", "s")], "extract": [("type", "T")], "freq": [("len", "l"), ("umi", "u")], "filter": [("len", "l"), ("seed", "s")],
        "sweep": [("seed", "s")], "cap": [("seed", "s")], "level": [("seed", "s")], "crb": []}
FLOATS = {"bam2db": [("cell", "c"), ("depth", "r")], "filter": [("rate", "t")]}
VALUED = {"bam2db": ("bam", "b"), "crb": ("out", "o"), "extract": ("tag", "t"), "freq": ("R1", "R"), "filter": ("whitelist", "w"),
          "sweep": ("barcode", "a"), "cap": ("reads", "n"), "level": ("umis", "m")}
# sha256 of the `-h` text
HELP = {"bam2db": "9d728b565cdc267a24d479b446d509e4c3019d8b4fc355bd3212912fdd1c0921", "crb": "5911484b3a6be838c79afa02d66d7267c8f3b7e1928f2da27056fdd61c0245d5",
        "extract": "14b35a173858ce4dc4b07b6db6e06a8341cf570e16cc9fe272af43c4fc8644ab", "freq": "44579900ae2746a66db10be67038bdad9248d776ffd89bd2841b9846416e1ce1",
        "filter": "58bddf0e017cf35ae1b0ec8cb63415caa6d6aa4c491bde8da49c408d553b349b", "sweep": "156b9585a27b803ff3ee2f48c1a36a6e90c56ae1053b12b9c376a976a5fef384",
        "cap": "50a2bb7b09d91176fd0d630413bf06bb6a70110f3ebb1a6a75efb5665b142ff2", "level": "f2a0aa969e4459e5fa5d28714a30cbd21914c812c8ada103a7041a5b984af5fe"}


@pytest.fixture(scope="module")
def cwd(tmp_path_factory):
    """an empty, writable directory that every command runs in, with one small R1 file"""
    d = tmp_path_factory.mktemp("cli_options")
    (d / "r1.fq").write_bytes(b"@r0\nACGTACGTACGTACGTACGTACGTAC\n+\nIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    return d


@pytest.fixture(scope="module")
def run(cwd):
    def run(cmd, *args):
        r = subprocess.run([_lib.cli_path(), cmd] + [str(a) for a in args], capture_output=True, text=True, cwd=cwd, timeout=60)
        return r.returncode, r.stdout, r.stderr
    return run


@pytest.fixture(scope="module")
def usage(run):
    """the `-h` text of every command"""
    out = {}
    for cmd in ALL:
        rc, so, se = run(cmd, "-h")
        assert (rc, se) == (0, "") and so.startswith("Usage: fastF %s [options]\n" % cmd)
        out[cmd] = so
    return out


def no_bam(path):
    return 1, "", RED + "bam file: %s does not exist.\n" % path


def behind_the_loop(cmd):
    """the triple of a run whose options all parsed and set nothing but numbers: the first check behind the loop"""
    return {"bam2db": no_bam("(null)"), "extract": no_bam("(null)"), "sweep": no_bam("(null)"),
            "crb": (1, "", RED + "path to bam file can not been NULL while extracting .\n"),
            "cap": (1, "", RED + "cap needs -n <list>: the reads per cell at most\n"),
            "level": (1, "", RED + "level needs -m <list>: the UMIs per cell at most\n"),
            "freq": (1, "", "Please specify the path to R1 fastq files.\n"),
            "filter": (1, "whitelist: (null)\n", RED + "path to R1 fastq files can not been NULL while filtering .\n")}[cmd]


def unknown(cmd, usage, arg):
    msg = "error: unknown option `%s`\n" % arg
    return {"stderr": (1, "", msg + usage[cmd]), "stdout": (1, usage[cmd], msg), None: (1, "", msg)}[USAGE[cmd]]


def spellings(long, short, value):
    """the four ways to hand an option its value, with the name each is reported by"""
    return [(["--" + long, value], "--" + long), (["--%s=%s" % (long, value)], "--" + long), (["-" + short, value], "-" + short), (["-" + short + value], "-" + short)]


@pytest.mark.parametrize("cmd", ALL)
def test_the_help_text(cmd, run, usage):
    assert hashlib.sha256(usage[cmd].encode()).hexdigest() == HELP[cmd]
    long, short = VALUED[cmd]
    for args in (["--help"], ["--help=x"], ["-" + short, "x", "-h"], ["--%s=x" % long, "--help"], ["-" + short + "x", "-h", "--bogus"]):
        assert run(cmd, *args) == (0, usage[cmd], ""), args


@pytest.mark.parametrize("cmd", ALL)
def test_unknown_options(cmd, run, usage):
    long, short = VALUED[cmd]
    for arg in ("--bogus", "-Z", "--bogus=1", "--" + long + "x", "--" + long + "x=1", "--" + long[:-1], "--=x", "---"):
        assert run(cmd, arg) == unknown(cmd, usage, arg), arg
        assert run(cmd, "-" + short, "x", arg, "-h") == unknown(cmd, usage, arg), arg


@pytest.mark.parametrize("cmd", GRID)
def test_the_long_only_options_of_the_grid_verbs_have_no_letter(cmd, run, usage):
    for letter in "SGCFQNXPTLMER":
        assert run(cmd, "-" + letter) == unknown(cmd, usage, "-" + letter), letter
        assert run(cmd, "-" + letter + "x") == unknown(cmd, usage, "-" + letter + "x"), letter
    # nor has a verb the list option of another
    for other in GRID:
        if other != cmd:
            long, short = VALUED[other] if other != "sweep" else ("depth", "r")
            assert run(cmd, "-" + short, "1") == unknown(cmd, usage, "-" + short)
            assert run(cmd, "--" + long, "1") == unknown(cmd, usage, "--" + long)


@pytest.mark.parametrize("cmd", ALL)
def test_a_missing_value(cmd, run):
    long, short = VALUED[cmd]
    pairs = [(long, short)] + INTS[cmd] + FLOATS.get(cmd, [])
    for lg, sh in pairs:
        assert run(cmd, "--" + lg) == (1, "", "error: option `--%s` requires a value\n" % lg)
        assert run(cmd, "-" + sh) == (1, "", "error: option `-%s` requires a value\n" % sh)
    # the options before it parsed; `--long=` is an empty value, not a missing one
    assert run(cmd, "-" + short, "x", "--" + long) == (1, "", "error: option `--%s` requires a value\n" % long)
    if cmd in GRID:
        for lg in ("pseudotime", "labels", "markers", "seeds", "reps"):
            assert run(cmd, "--genes", "--" + lg) == (1, "", "error: option `--%s` requires a value\n" % lg)


@pytest.mark.parametrize("cmd", [c for c in ALL if INTS[c]])
def test_integer_values(cmd, run):
    for long, short in INTS[cmd]:
        for bad in ("12x", "x", "1.5", "=5", "0x", "08"):
            for args, name in spellings(long, short, bad):
                assert run(cmd, *args) == (1, "", "error: option `%s` expects an integer value\n" % name), args
        for args, name in spellings(long, short, HUGE) + spellings(long, short, "-" + HUGE):
            if cmd == "extract":                               # -T has no range check: the run goes on
                assert run(cmd, *args) == behind_the_loop(cmd), args
            else:
                assert run(cmd, *args) == (1, "", "error: option `%s` numerical result out of range\n" % name), args
        # the range is looked at before the trailing characters
        if cmd != "extract":
            assert run(cmd, "--" + long, HUGE + "x") == (1, "", "error: option `--%s` numerical result out of range\n" % long)
        # an empty value is 0; the base is taken from the prefix; the value may begin with `-`
        for good in ("", "0x1F", "017", "-3", " 7"):
            for args, _ in spellings(long, short, good)[:3] + ([] if good == "" else spellings(long, short, good)[3:]):
                assert run(cmd, *args) == behind_the_loop(cmd), args


@pytest.mark.parametrize("cmd", sorted(FLOATS))
def test_float_values(cmd, run):
    for long, short in FLOATS[cmd]:
        for bad in ("0.5x", "x", "=1", "1e"):
            for args, name in spellings(long, short, bad):
                assert run(cmd, *args) == (1, "", "error: option `%s` expects a numerical value\n" % name), args
        for bad in ("1e99", "-1e99", "1e99x", "1e-99"):
            for args, name in spellings(long, short, bad):
                assert run(cmd, *args) == (1, "", "error: option `%s` numerical result out of range\n" % name), args
        for good in ("", "0.5", "1e3", "-2", "0x1p-1", "inf", "nan"):
            for args, _ in spellings(long, short, good)[:3] + ([] if good == "" else spellings(long, short, good)[3:]):
                assert run(cmd, *args) == behind_the_loop(cmd), args


@pytest.mark.parametrize("cmd", ("bam2db", "extract") + GRID)
def test_the_value_of_bam_reaches_its_field(cmd, run):
    for args, _ in spellings("bam", "b", "/no/such"):
        assert run(cmd, *(LIST[cmd] + args)) == no_bam("/no/such"), args
        assert run(cmd, *(args + LIST[cmd])) == no_bam("/no/such"), args
        assert run(cmd, *(LIST[cmd] + ["-b", "A"] + args)) == no_bam("/no/such"), args           # the last one wins
    assert run(cmd, *(LIST[cmd] + ["-b", "-f"])) == no_bam("-f")                                 # a value may look like an option
    assert run(cmd, *(LIST[cmd] + ["--bam", "--bam"])) == no_bam("--bam")
    assert run(cmd, *(LIST[cmd] + ["--bam="])) == no_bam("")


def test_the_values_of_bam2db_and_the_grid_verbs_reach_their_fields(run, cwd):
    (cwd / "here").write_bytes(b"")
    for cmd in ("bam2db",) + GRID:
        more = LIST[cmd]
        assert run(cmd, *more, "-b", "here", "--feature=/no/f") == (1, "", RED + "feature file: /no/f does not exist.\n")
        assert run(cmd, *more, "-b", "here", "-fhere", "-a", "/no/a") == (1, "", RED + "barcode file: /no/a does not exist.\n")
        assert run(cmd, *more, "-b", "here", "-fhere", "--barcode", "/no/a", "-d", "x", "-dx", "--dbname=x", "-o", "x", "-c", "1") == \
            (1, "", RED + "barcode file: /no/a does not exist.\n")
    assert run("bam2db", "-b", "here", "-f", "here", "-a", "here", "--dbname", "here") == \
        (1, "", RED + "database: here already exists, change the name of database in -d argument!\n")
    # a flag ignores what is glued behind its letter and what follows its long name's `=`
    assert run("bam2db", "-uZZ", "--umicopies", "--umicopies=1", "-b", "/no/such") == no_bam("/no/such")
    for cmd in GRID:
        u = {"sweep": "sweep does not write umi.tsv.gz (-u): run bam2db -u for the points that need it.", "cap": "cap does not write umi.tsv.gz (-u).",
             "level": "level does not write umi.tsv.gz (-u)."}[cmd]
        for arg in ("-u", "-uZZ", "--umicopies", "--umicopies=1"):
            assert run(cmd, "-b", "x", arg, "--bogus") == (1, "", RED + u + "\n"), arg
        # the list option by both names, the cell rates, and the long-only options with a value
        lg, sh = {"sweep": ("depth", "r"), "cap": ("reads", "n"), "level": ("umis", "m")}[cmd]
        bad = {"sweep": "depth rates", "cap": "reads per cell", "level": "level: UMIs per cell"}[cmd] + " `1,,2`: empty element"
        for args, _ in spellings(lg, sh, "1,,2"):
            assert run(cmd, *args) == (1, "", RED + bad + "\n"), args
        for args, _ in spellings("cell", "c", "1,,2"):
            assert run(cmd, *(LIST[cmd] + args)) == (1, "", RED + "cell rates `1,,2`: empty element\n"), args
        assert run(cmd, "--genes", "--cells=1", "--summary-only", "--fidelity", "--gene-fidelity", "--neighbors", "--coexpression", "--mapping", "--pseudotime", "p",
                   "--labels=l", "--markers", "0") == (1, "", "error: option `--markers` expects an integer from 1 to 2000\n")
        assert run(cmd, "--markers=12x", "--labels", "l") == (1, "", "error: option `--markers` expects an integer from 1 to 2000\n")
        assert run(cmd, "--markers=3") == (1, "", "error: option `--markers` needs `--labels`\n")
        assert run(cmd, "--reps=0") == (1, "", "error: option `--reps` expects an integer from 1 to 64\n")
        assert run(cmd, "--reps", "") == (1, "", "error: option `--reps` expects an integer from 1 to 64\n")
        assert run(cmd, "--seeds=7,7") == (1, "", "error: option --seeds `7,7`: 7 is listed twice\n")
        assert run(cmd, "--seeds", "7", "--reps", "2") == (1, "", "error: option `--seeds` cannot be combined with `--reps`\n")
        for args, _ in spellings("seed", "s", "3"):
            assert run(cmd, "--seeds", "7", *args) == (1, "", "error: option `--seeds` cannot be combined with `-s`\n"), args


def test_the_values_of_crb_and_extract_reach_their_fields(run, cwd):
    for args, _ in spellings("out", "o", "/no/such/dir/x"):
        assert run("crb", "-b", "x", *args) == (1, "", RED + "can not open file /no/such/dir/x\n"), args
        assert run("crb", *args) == behind_the_loop("crb"), args
        assert run("crb", "-o", "A", "--bam=x", *args) == (1, "", RED + "can not open file /no/such/dir/x\n"), args
    assert not (cwd / "A").exists()
    assert run("crb", "-hZZ") == run("crb", "-h")
    (cwd / "here").write_bytes(b"")
    assert run("extract", "-b", "here") == (1, "", RED + "--tag is required.\n")
    assert run("extract", "-b", "here", "-T", "1", "--type=0") == (1, "", RED + "--tag is required.\n")
    for args, _ in spellings("tag", "t", "CB"):
        assert run("extract", *args) == no_bam("(null)"), args
    assert run("extract", "-T", HUGE) == no_bam("(null)")


def test_the_values_of_freq_reach_their_fields(run):
    for args, _ in spellings("R1", "R", "/no/such"):
        assert run("freq", *args) == (1, "", "Cannot open file /no/such \n"), args
        assert run("freq", "-R", "A", *args) == (1, "", "Cannot open file /no/such \n"), args
        assert run("freq", *args, "-l", "16", "--umi=10", "-o", "x") == (1, "", "Cannot open file /no/such \n"), args
    assert run("freq", "-R", "-l") == (1, "", "Cannot open file -l \n")
    for args, _ in spellings("out", "o", "/no/such/dir"):
        assert run("freq", "-R", "r1.fq", *args) == (1, "", "Cannot open file /no/such/dir/whitelist.txt \n"), args
    assert run("freq", "-R", "r1.fq") == (1, "", "Cannot open file (null)/whitelist.txt \n")


def test_the_values_of_filter_reach_their_fields(run):
    no_r1 = RED + "path to R1 fastq files can not been NULL while filtering .\n"
    for args, _ in spellings("whitelist", "w", "X"):
        assert run("filter", *args) == (1, "whitelist: X\n", no_r1), args
        assert run("filter", "-w", "A", *args) == (1, "whitelist: X\n", no_r1), args
    for args, _ in spellings("R1", "R", "/no/such"):
        assert run("filter", "-a", *args) == (1, "whitelist: (null)\n", "Cannot open file /no/such \n"), args
        assert run("filter", *args) == (1, "whitelist: (null)\n", RED + "whitelist and --all cell option can not been both NULL at the same time.\n"), args
    for flag in ("-a", "--allcells", "--allcells=x"):
        assert run("filter", flag, "-R", "/no/such") == (1, "whitelist: (null)\n", "Cannot open file /no/such \n"), flag
    for long, short in (("I1", "I"), ("R2", "r")):
        for args, _ in spellings(long, short, "/no/mate"):
            assert run("filter", "-a", "-R", "r1.fq", *args)[::2] == (1, "Cannot open file /no/mate \n"), args
    for args, _ in spellings("out", "o", "/no/such/dir"):
        assert run("filter", "-a", "-R", "r1.fq", *args) == \
            (1, "whitelist: (null)\n", RED + "cannot write the outputs into directory /no/such/dir (gzopen would return NULL; refused)\n"), args
    # the length reaches its field as an int: the refusal prints it
    for value, n in (("-5", -5), ("-0x5", -5), ("-2147483648", -2147483648), ("4294967291", -5)):
        for args, _ in spellings("len", "l", value):
            assert run("filter", "-a", "-R", "r1.fq", *args) == \
                (1, "whitelist: (null)\n", RED + "-l %d: negative length of cell barcode (malloc(%d) in substring, filter.c:262; refused)\n" % (n, n + 1)), args


@pytest.mark.parametrize("cmd", STOP)
def test_the_stop_dialect(cmd, run):
    """the first argument that is no option, a lone `-` and `--` end the parsing: what follows is never looked at"""
    for stop in ("stray", "-", "--", ""):
        assert run(cmd, stop, "-b", "/no/such", "--bogus", "-h") == behind_the_loop(cmd), stop
        if cmd == "crb":
            assert run(cmd, "-b", "x", "-o", "/no/such/dir/x", stop, "-o", "y", "--bogus") == (1, "", RED + "can not open file /no/such/dir/x\n"), stop
        else:
            assert run(cmd, *LIST[cmd], "-b", "/no/such", stop, "-b", "/other", "--bogus") == no_bam("/no/such"), stop
    # no clusters: a valued option takes everything behind its letter, `-s=5` is the value `=5`
    if INTS[cmd]:
        long, short = INTS[cmd][0]
        assert run(cmd, "-%s=5" % short) == (1, "", "error: option `-%s` expects an integer value\n" % short)
        assert run(cmd, "-%s5h" % short) == (1, "", "error: option `-%s` expects an integer value\n" % short)
    if cmd != "crb":
        assert run(cmd, *LIST[cmd], "-bh") == no_bam("h")


@pytest.mark.parametrize("cmd", ARGPARSE)
def test_the_argparse_dialect(cmd, run, usage):
    """arguments that are no options are skipped, `--` ends the parsing, the short options cluster"""
    bad_r1 = {"freq": (1, "", "Cannot open file /no/such \n"), "filter": (1, "whitelist: (null)\n", "Cannot open file /no/such \n")}[cmd]
    a = [] if cmd == "freq" else ["-a"]
    for skipped in ("stray", "-", ""):
        assert run(cmd, skipped, *a, skipped, "-R", "/no/such", skipped) == bad_r1, skipped
        assert run(cmd, skipped, "-h") == (0, usage[cmd], "")
        assert run(cmd, skipped, "--bogus") == unknown(cmd, usage, "--bogus")
    assert run(cmd, "--", "-R", "/no/such", "--bogus", "-h") == behind_the_loop(cmd)
    if cmd == "freq":
        assert run(cmd, "-R", "/no/such", "--", "-R", "/other") == bad_r1
        assert run(cmd, "-l", "16", "--", "-h") == behind_the_loop(cmd)
    else:
        assert run(cmd, "-a", "-R", "/no/such", "--", "-R", "/other") == bad_r1
    # a long name is followed by nothing or by `=`
    for arg in ("--R1x", "--R1x=1", "--R", "--len16", "--helpx"):
        assert run(cmd, arg, "/no/such") == unknown(cmd, usage, arg), arg
    # clusters: the rest of a cluster is the value of the first option that takes one; an unknown letter names the whole argument
    assert run(cmd, "-l16", "-R/no/such", *a) == bad_r1
    assert run(cmd, "-l=5") == (1, "", "error: option `-l` expects an integer value\n")
    assert run(cmd, "-l5h") == (1, "", "error: option `-l` expects an integer value\n")
    assert run(cmd, "-lh") == (1, "", "error: option `-l` expects an integer value\n")
    assert run(cmd, "-Zh") == unknown(cmd, usage, "-Zh")
    assert run(cmd, "-hZ") == (0, usage[cmd], "")
    if cmd == "filter":
        no_r1 = RED + "path to R1 fastq files can not been NULL while filtering .\n"
        assert run(cmd, "-aw", "X") == (1, "whitelist: X\n", no_r1)
        assert run(cmd, "-aawX") == (1, "whitelist: X\n", no_r1)
        assert run(cmd, "-aR", "/no/such") == bad_r1
        assert run(cmd, "-aR/no/such") == bad_r1
        assert run(cmd, "-al16", "-R", "/no/such") == bad_r1
        assert run(cmd, "-al16x") == (1, "", "error: option `-l` expects an integer value\n")
        assert run(cmd, "-al" + HUGE) == (1, "", "error: option `-l` numerical result out of range\n")
        assert run(cmd, "-at0.5x") == (1, "", "error: option `-t` expects a numerical value\n")
        assert run(cmd, "-al") == (1, "", "error: option `-l` requires a value\n")
        assert run(cmd, "-aZ") == unknown(cmd, usage, "-aZ")
        assert run(cmd, "-aZw", "X") == unknown(cmd, usage, "-aZw")
        assert run(cmd, "-ah") == (0, usage[cmd], "")
        assert run(cmd, "-aha", "--bogus") == (0, usage[cmd], "")
        assert run(cmd, "-wXh") == (1, "whitelist: Xh\n", no_r1)
