"""The way into the grid driver of sweep, cap and level, without a device: the six entry points of a verb, the Python functions and the
command.  No run here reaches a device, so what is pinned is the message of every refusal, word for word, that the calls the header
documents as reductions of each other give the same one, the order of the checks, and that a refusal leaves no output directory."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, level, sweep
import test_gpu_ptime as TP
import test_labels_host as LH

VERBS = ("sweep", "cap", "level")
MOD = {"sweep": sweep, "cap": cap, "level": level}
OPT = {"sweep": "-r", "cap": "-n", "level": "-m"}
VALUES = {"sweep": [0.5, 1], "cap": [3, 8], "level": [2, 6]}
UNASSIGNED = (4, 16, 64, 256, 1024, 2048, 8192)
ASSIGNED = 1 | 2 | 8 | 32 | 128 | 512 | 4096
RED = "\x1b[31mError:\x1b[0m "


def _call(verb, kind, bam, out, barcodes=b"b", features=b"f", rates=(1,), values=None, flags=0, seeds=None, seed=926, labels=None, markers=0,
          mapping=0, ptime=None):
    """the message of fastf_<verb>[_<kind>] through the raw symbol, "" where it returned 0"""
    L = _lib.lib()
    enc = lambda p: None if p is None else os.fspath(p).encode() if not isinstance(p, bytes) else p  # noqa: E731
    rc, prc = sweep._floats(rates)
    lv = np.ascontiguousarray(VALUES[verb] if values is None else values, np.float32 if verb == "sweep" else np.uint64)
    plv = lv.ctypes.data_as(C.POINTER(C.c_float)) if verb == "sweep" else lv.ctypes.data
    sd = np.ascontiguousarray([] if seeds is None else seeds, np.uint32)
    psd = None if seeds is None else sd.ctypes.data
    head = (enc(bam), enc(out), enc(barcodes), enc(features), prc, len(rc), plv, len(lv))
    fn = getattr(L, "fastf_%s%s" % (verb, "_" + kind if kind else ""))
    if kind == "":
        r = fn(*head, seed, flags)
    elif kind == "reps":
        r = fn(*head, psd, len(sd), flags)
    else:
        tail = {"labels": (enc(labels),), "markers": (enc(labels), markers), "mapping": (enc(labels), markers, mapping),
                "pseudotime": (enc(labels), markers, mapping, enc(ptime))}[kind]
        r = fn(*head, psd, len(sd), flags, seed, *tail)
    assert r in (0, 1)
    return L.fastf_last_error().decode() if r else ""


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the synthetic BAM of the labels tests with its lists, its labels file and its pseudotime file"""
    d = tmp_path_factory.mktemp("grid_entry")
    return (d,) + TP._write(d, LH.labcase())


def _scenarios(files):
    """(what stops the run, the arguments that make it, the message every call must give): a missing BAM, and each unassigned flag bit
    on files that exist — both are found before a device is looked for"""
    d, bam, b, f, lf, pf = files
    missing = d / "missing.bam"
    yield "a missing BAM", dict(bam=missing, barcodes=b, features=f), "bam file: %s does not exist." % missing
    for bit in UNASSIGNED:
        for flags in (bit, bit | ASSIGNED):
            yield "flag bit %d" % bit, dict(bam=bam, barcodes=b, features=f, flags=flags), "%%s: unknown flags 0x%x" % flags


@pytest.mark.parametrize("verb", VERBS)
def test_the_documented_reductions_give_the_message_of_the_lower_call(verb, files):
    d, bam, b, f, lf, pf = files
    out = d / ("out_reductions_" + verb)
    for what, kw, want in _scenarios(files):
        want = want % verb if "%s" in want else want
        kw = dict(kw, out=out)
        for seeds in (None, [7, 8]):
            for labels, markers in ((None, 0), (lf, 0), (lf, 3)):
                for mapping in (0, 1):
                    # _pseudotime(NULL) is _mapping
                    got = _call(verb, "mapping", seeds=seeds, labels=labels, markers=markers, mapping=mapping, **kw)
                    assert got == want, (what, seeds, labels, markers, mapping)
                    assert _call(verb, "pseudotime", seeds=seeds, labels=labels, markers=markers, mapping=mapping, ptime=None, **kw) == got
                    assert _call(verb, "pseudotime", seeds=seeds, labels=labels, markers=markers, mapping=mapping, ptime=pf, **kw) == got
                # _mapping(mapping = 0) is _markers with markers != 0, else _labels
                lower = _call(verb, "markers", seeds=seeds, labels=labels, markers=markers, **kw) if markers else _call(verb, "labels", seeds=seeds, labels=labels, **kw)
                assert lower == want == _call(verb, "mapping", seeds=seeds, labels=labels, markers=markers, mapping=0, **kw), (what, seeds, labels, markers)
            # _labels(NULL) with n_seeds = 0 is the plain call at `seed`, with n_seeds = k the replicate call
            lower = _call(verb, "", **kw) if seeds is None else _call(verb, "reps", seeds=seeds, **kw)
            assert lower == want == _call(verb, "labels", seeds=seeds, labels=None, **kw), (what, seeds)
        # seeds given with n_seeds = 0 is the plain call too, for the four calls that take `seed`
        for kind in ("labels", "markers", "mapping", "pseudotime"):
            assert _call(verb, kind, seeds=[], labels=lf, markers=3, **kw) == want, (what, kind)
    assert not out.exists()


@pytest.mark.parametrize("verb", VERBS)
def test_the_refusals_of_the_entry_points_and_their_order(verb, files):
    d, bam, b, f, lf, pf = files
    out = d / ("out_refusals_" + verb)
    missing = d / "missing.bam"
    no_bam = "bam file: %s does not exist." % missing
    kw = dict(bam=missing, out=out, barcodes=b, features=f)
    # --mapping beyond 1 comes first: before a bad N of --markers, before the seeds, before the grid
    for kind in ("mapping", "pseudotime"):
        for more in (dict(), dict(markers=2001, labels=lf), dict(markers=5), dict(seeds=[7, 7]), dict(rates=[]), dict(values=[])):
            assert _call(verb, kind, mapping=2, **dict(kw, **more)) == "%s: --mapping: 2, 0 or 1" % verb, (kind, more)
        assert _call(verb, kind, mapping=0xFFFFFFFF, **kw) == "%s: --mapping: 4294967295, 0 or 1" % verb
    # _markers: N from 1 to 2000 and a labels path, always; before the seeds and the grid
    for n in (0, 2001):
        for more in (dict(labels=lf), dict(labels=None), dict(labels=lf, seeds=[7, 7]), dict(labels=lf, rates=[])):
            assert _call(verb, "markers", markers=n, **dict(kw, **more)) == "%s: --markers: N = %d, from 1 to 2000" % (verb, n), (n, more)
    assert _call(verb, "markers", markers=5, labels=None, **kw) == "%s: --markers needs --labels" % verb
    assert _call(verb, "markers", markers=2000, labels=lf, **kw) == _call(verb, "markers", markers=1, labels=lf, **kw) == no_bam
    # _mapping and _pseudotime: the same two checks with markers != 0 only
    for kind in ("mapping", "pseudotime"):
        assert _call(verb, kind, markers=2001, labels=lf, **kw) == "%s: --markers: N = 2001, from 1 to 2000" % verb
        assert _call(verb, kind, markers=5, labels=None, **kw) == "%s: --markers needs --labels" % verb
        assert _call(verb, kind, markers=5, labels=None, seeds=[7, 7], **kw) == "%s: --markers needs --labels" % verb
        assert _call(verb, kind, markers=0, labels=None, **kw) == _call(verb, kind, markers=0, labels=lf, **kw) == no_bam
    # the seeds of a replicate run: 1 to 64 distinct values, checked before the null arguments and the grid
    takes = "%s: a replicate run takes 1 to 64 seeds" % verb
    assert _call(verb, "reps", seeds=[], **kw) == takes == _call(verb, "reps", seeds=list(range(65)), **kw)
    assert _call(verb, "reps", seeds=None, **kw) == takes
    assert _call(verb, "reps", seeds=list(range(64)), **kw) == no_bam == _call(verb, "reps", seeds=[0xFFFFFFFF], **kw)
    for kind in ("reps", "labels", "markers", "mapping", "pseudotime"):
        more = dict(labels=lf, markers=3) if kind != "reps" else {}
        assert _call(verb, kind, seeds=[7, 8, 7], **dict(kw, **more)) == "%s: seed 7 is listed twice" % verb
        assert _call(verb, kind, seeds=list(range(65)), **dict(kw, **more)) == takes
        assert _call(verb, kind, seeds=[7, 7], rates=[], **dict(kw, **more)) == "%s: seed 7 is listed twice" % verb
        assert _call(verb, kind, seeds=[7, 7], **dict(kw, bam=None, **more)) == "%s: seed 7 is listed twice" % verb
    for kind in ("", "reps", "labels", "markers", "mapping", "pseudotime"):
        more = dict(labels=lf, markers=3) if kind not in ("", "reps") else {}
        more = dict(more, seeds=[7]) if kind == "reps" else more
        assert _call(verb, kind, **dict(kw, bam=None, **more)) == "%s: null argument" % verb
        assert _call(verb, kind, **dict(kw, features=None, **more)) == "%s: null argument" % verb
    # with a labels path the BAM is looked for before the labels are read; then the labels, then the grid
    assert _call(verb, "labels", labels=d / "no.labels", **kw) == no_bam
    assert _call(verb, "labels", labels=lf, rates=[], **dict(kw, bam=bam)).startswith("%s: the grid needs at least one cell rate and one " % verb)
    assert _call(verb, "pseudotime", ptime=d / "no.ptime", **kw) == no_bam
    assert not out.exists()


@pytest.mark.parametrize("verb", VERBS)
def test_a_bad_grid_is_refused_by_every_entry_point_alike(verb, files):
    d, bam, b, f, lf, pf = files
    out = d / ("out_grid_" + verb)
    kw = dict(bam=bam, out=out, barcodes=b, features=f)
    unit = {"sweep": "depth rate", "cap": "cap", "level": "cap"}[verb]
    dup = {"sweep": "sweep: depth rates 0.5 and 0.5001 both print as 0.500", "cap": "cap: reads per cell 7 is listed twice",
           "level": "level: UMIs per cell 7 is listed twice"}[verb]
    zero = {"sweep": None, "cap": "cap: reads per cell 0: a cap is at least 1", "level": "level: UMIs per cell 0: a cap is at least 1"}[verb]
    cases = [(dict(rates=[]), "%s: the grid needs at least one cell rate and one %s" % (verb, unit)),
             (dict(values=[]), "%s: the grid needs at least one cell rate and one %s" % (verb, unit)),
             (dict(rates=[0.25, 0.2501]), "%s: cell rates 0.25 and 0.2501 both print as 0.250" % verb),
             (dict(rates=[1.5]), "%s: cell rate 1.5: sample size must lie in [0, number of barcodes]" % verb),
             (dict(rates=[-0.5]), "%s: cell rate -0.5 is negative or not a number" % verb),
             (dict(values=[0.5, 0.5001] if verb == "sweep" else [7, 3, 7]), dup)]
    if zero:
        cases.append((dict(values=[3, 0]), zero))
    else:
        cases.append((dict(values=[-1.0]), "sweep: depth rate -1 is negative or not a number"))
    for more, want in cases:
        got = {kind: _call(verb, kind, **dict(kw, **more, **(dict(seeds=[7]) if kind == "reps" else {}), **(dict(labels=lf, markers=3) if kind not in ("", "reps") else {})))
               for kind in ("", "reps", "labels", "markers", "mapping", "pseudotime")}
        assert set(got.values()) == {want}, (more, got)
        assert _call(verb, "pseudotime", labels=lf, markers=3, mapping=1, ptime=pf, seeds=[7, 8], flags=ASSIGNED, **dict(kw, **more)) == want
    # the grid comes before the flags, the flags before the BAM
    assert _call(verb, "", flags=4, **dict(kw, rates=[])).startswith("%s: the grid needs" % verb)
    assert _call(verb, "", flags=4, **dict(kw, bam=d / "missing.bam")) == "%s: unknown flags 0x4" % verb
    # a rate of 0 is a grid like any other: the run goes on to the next check
    assert _call(verb, "", rates=[0.0], **dict(kw, bam=d / "missing.bam")) == "bam file: %s does not exist." % (d / "missing.bam")
    assert not out.exists()


@pytest.mark.parametrize("verb", VERBS)
def test_python_hands_a_bad_markers_to_the_markers_call_whatever_else_is_set(verb, files):
    d, bam, b, f, lf, pf = files
    out = d / ("out_python_" + verb)
    missing = d / "missing.bam"
    plain, reps = MOD[verb].__dict__[verb], MOD[verb].__dict__[verb + "_reps"]
    for bad in ("x", 0, 2 ** 32, -1, 2.5, (3,)):
        for mapping in (False, True):
            for ptime in (None, pf):
                for labels in (None, lf):
                    for fn, extra in ((plain, dict(seed=5)), (reps, dict(seeds=[7, 8]))):
                        with pytest.raises(F.FastfError) as ei:
                            fn(missing, out, b, f, [1], VALUES[verb], markers=bad, mapping=mapping, pseudotime=ptime, labels=labels, **extra)
                        assert str(ei.value) == "%s: --markers: N = 0, from 1 to 2000" % verb, (bad, mapping, ptime, labels)
    # every other combination of the options reaches the driver: here its look for the BAM
    for markers, labels, want in ((None, None, None), (None, lf, None), (3, lf, None), (3, None, "%s: --markers needs --labels" % verb),
                                  (2001, lf, "%s: --markers: N = 2001, from 1 to 2000" % verb)):
        for mapping in (False, True):
            for ptime in (None, pf):
                for fn, extra in ((plain, dict()), (reps, dict(seeds=[7])), (reps, dict(seeds=range(3)))):
                    with pytest.raises(F.FastfError) as ei:
                        fn(missing, out, b, f, [1], VALUES[verb], markers=markers, mapping=mapping, pseudotime=ptime, labels=labels, cells=True, **extra)
                    assert str(ei.value) == (want or "bam file: %s does not exist." % missing), (markers, labels, mapping, ptime)
    # the seeds of a replicate call
    with pytest.raises(F.FastfError) as ei:
        reps(missing, out, b, f, [1], VALUES[verb], [])
    assert str(ei.value) == "%s: a replicate run takes 1 to 64 seeds" % verb
    for kw in (dict(), dict(labels=lf), dict(labels=lf, markers=3), dict(mapping=True), dict(pseudotime=pf)):
        with pytest.raises(F.FastfError) as ei:
            reps(missing, out, b, f, [1], VALUES[verb], [7, 2 ** 32 + 7], **kw)
        assert str(ei.value) == "%s: seed 7 is listed twice" % verb
    with pytest.raises(F.FastfError) as ei:
        plain(missing, out, b, f, [1], VALUES[verb], fidelity=True, gene_fidelity=True, neighbors=True, coexpression=True, genes=True, summary_only=True)
    assert str(ei.value) == "bam file: %s does not exist." % missing
    assert not out.exists()


def _cli(verb, *args, env=None):
    return subprocess.run([_lib.cli_path(), verb] + [str(a) for a in args], capture_output=True, text=True, env=env)


@pytest.mark.parametrize("verb", VERBS)
def test_the_messages_of_the_command_and_no_output_directory_behind_a_refusal(verb, files):
    d, bam, b, f, lf, pf = files
    out = d / ("out_cli_" + verb)
    io = ["-b", bam, "-a", b, "-f", f, "-o", out]
    grid = ["-c", "1", OPT[verb], ",".join(str(v) for v in VALUES[verb])]
    u = {"sweep": "sweep does not write umi.tsv.gz (-u): run bam2db -u for the points that need it.", "cap": "cap does not write umi.tsv.gz (-u).",
         "level": "level does not write umi.tsv.gz (-u)."}[verb]
    for args in (io + grid + ["-u"], ["-u"], ["--umicopies"] + io):
        r = _cli(verb, *args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", RED + u + "\n")
    r = _cli(verb, "-b", d / "missing.bam", "-c", "1")      # the list is missed before an input file is looked for; sweep's defaults to 1
    needs = {"sweep": "bam file: %s does not exist." % (d / "missing.bam"), "cap": "cap needs -n <list>: the reads per cell at most",
             "level": "level needs -m <list>: the UMIs per cell at most"}[verb]
    assert (r.returncode, r.stdout, r.stderr) == (1, "", RED + needs + "\n")
    r = _cli(verb, "--seeds", "7,7")                        # the options are read first
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "error: option --seeds `7,7`: 7 is listed twice\n")
    # the list and the grid, then the three input files, then the run
    bad_list = {"sweep": ("0.5,,1", "depth rates `0.5,,1`: empty element"), "cap": ("3,x", "reads per cell `3,x`: expects positive integers"),
                "level": ("3,x", "level: UMIs per cell `3,x`: expects positive integers")}[verb]
    r = _cli(verb, "-b", d / "missing.bam", "-c", "1", OPT[verb], bad_list[0])
    assert (r.returncode, r.stdout, r.stderr) == (1, "", RED + bad_list[1] + "\n")
    r = _cli(verb, *(io + ["-c", "0.25,0.2501", OPT[verb], "1"]))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", RED + "%s: cell rates 0.25 and 0.2501 both print as 0.250\n" % verb)
    r = _cli(verb, "-b", d / "missing.bam", "-a", b, "-f", f, "-o", out, *grid)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", RED + "bam file: %s does not exist.\n" % (d / "missing.bam"))
    r = _cli(verb, "-b", bam, "-a", d / "missing.tsv", "-f", f, "-o", out, *grid)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", RED + "barcode file: %s does not exist.\n" % (d / "missing.tsv"))
    # what the parser refuses of --markers and --mapping never reaches an entry point
    r = _cli(verb, *(io + grid + ["--markers", "5"]))
    assert (r.returncode, r.stderr) == (1, "error: option `--markers` needs `--labels`\n")
    for n in ("0", "2001", "x"):
        r = _cli(verb, *(io + grid + ["--labels", lf, "--markers", n]))
        assert (r.returncode, r.stderr) == (1, "error: option `--markers` expects an integer from 1 to 2000\n")
    # a refusal of the driver comes back as "<verb> failed: ..."
    r = _cli(verb, *(io + grid + ["--labels", d / "no.labels", "--markers", "3", "--mapping", "--pseudotime", pf, "--seeds", "7,8"]))
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith(RED + "%s failed: " % verb) and "no.labels" in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("verb", VERBS)
def test_the_command_fails_by_name_where_no_device_is_to_be_had(verb, files):
    """every device hidden from the child: the most general run gets as far as the device and comes back as `<verb> failed: ...`, with
    no table, no point directory and nothing half written behind it"""
    d, bam, b, f, lf, pf = files
    out = d / ("out_nodevice_" + verb)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    for seeds in (["-s", "7"], ["--seeds", "7,8"]):
        r = _cli(verb, "-b", bam, "-a", b, "-f", f, "-o", out, "-c", "1", OPT[verb], ",".join(str(v) for v in VALUES[verb]), "--genes", "--cells", "--fidelity",
                 "--gene-fidelity", "--neighbors", "--coexpression", "--labels", lf, "--markers", "3", "--mapping", "--pseudotime", pf, *seeds, env=env)
        assert r.returncode == 1 and r.stderr.startswith(RED + "%s failed: " % verb) and "is generated" not in r.stdout, (r.stdout, r.stderr)
        assert not out.exists() or os.listdir(out) == []


# sha256 of " ".join(help.split()) of `fastF <verb> --help`: the words of a help text and their order, whatever its line breaks
HELP_WORDS = {"sweep": "a45530239d31b9f59814f7a48c3d9ba6e83738d7cdc64ed14977ee4d9641be3b", "cap": "92e459a872aa77203df8ef8dd4c03e0dec71d0c1bb884d11c1413e7e79b81ca9",
              "level": "6de00b8e4ca58da1f6ef907c928b20f096f15947bf1773afd4f9118b3bdd81a2"}


@pytest.mark.parametrize("verb", VERBS)
def test_the_words_of_the_help_text(verb):
    r = _cli(verb, "--help")
    assert r.returncode == 0 and r.stderr == ""
    assert hashlib.sha256(" ".join(r.stdout.split()).encode()).hexdigest() == HELP_WORDS[verb]
    assert _cli(verb, "-h").stdout == r.stdout
    bad = _cli(verb, "--bogus")                              # an unknown option: the same text on stderr behind its message
    assert bad.returncode == 1 and bad.stdout == "" and bad.stderr == "error: unknown option `--bogus`\n" + r.stdout
