"""The spellings of the options on the MI355X: freq, filter, extract and cap each run twice on the same small input, once with every
option in its plainest form (`-l 12`) and once in the unusual ones (`-l12`, `--len=0xc`, a cluster, a skipped argument), and leave
the same files, content byte for byte (the gzipped ones decompressed).  That a converted number reaches the device run is seen in the
output itself: the key length of freq, the restatement of filter, the integer tag of extract, the seed directories of cap."""
import gzip
import os
import random
import subprocess

import pytest

from fastf_amd import _lib

import filter_ref as R
import test_gpu_freq as TF
import test_gpu_labels as TL
import test_gpu_ptime as TP
import test_labels_host as LH
from tag_helpers import TagCase

pytestmark = pytest.mark.gpu


def _run(cmd, args, cwd):
    r = subprocess.run([_lib.cli_path(), cmd] + [str(a) for a in args], capture_output=True, text=True, cwd=cwd, timeout=300)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout


def _content(root):
    return {n: gzip.decompress(v) if n.endswith(".gz") else v for n, v in TL._tree(root).items()}


def test_freq(tmp_path):
    p = tmp_path / "in.fq"
    p.write_bytes(TF.fastq_text(TF.rand_seqs(random.Random(5), 3000, 26, n_distinct=300)))
    os.makedirs(tmp_path / "plain"), os.makedirs(tmp_path / "odd")
    _run("freq", ["-R", p, "-o", "plain", "-l", "12", "-u", "8"], tmp_path)
    _run("freq", ["stray", "--R1=%s" % p, "-oodd", "-", "--len=0xc", "-u010", "--", "-l", "3"], tmp_path)
    want = (tmp_path / "plain" / "whitelist.txt").read_bytes()
    assert (tmp_path / "odd" / "whitelist.txt").read_bytes() == want
    rows = want.split(b"\n")[:-1]
    assert rows and all(len(r.rpartition(b",")[0]) == 12 + 8 for r in rows) and sum(int(r.rpartition(b",")[2]) for r in rows) == 3000


def test_filter(tmp_path):
    texts, pool = R.tenx_triple(3000, seed=5, n_cells=40, p_other=0.3)
    paths = {n: tmp_path / (n + ".fq") for n in R.NAMES}
    for n in R.NAMES:
        paths[n].write_bytes(texts[n])
    wl_bytes = b"".join(b + b"\n" for b in pool[::2])
    (tmp_path / "wl.txt").write_bytes(wl_bytes)
    os.makedirs(tmp_path / "plain"), os.makedirs(tmp_path / "odd")
    so = _run("filter", ["-I", paths["I1"], "-R", paths["R1"], "-r", paths["R2"], "-o", "plain", "-w", "wl.txt", "-l", "14", "-s", "77", "-t", "0.5", "-a"], tmp_path)
    so2 = _run("filter", ["stray", "--I1=%s" % paths["I1"], "--R1", paths["R1"], "-r%s" % paths["R2"], "--out=odd", "-wwl.txt", "-l0xe", "--seed=0x4d", "-at5e-1",
                          "--", "-s", "1"], tmp_path)
    assert so2 == so
    want = R.read_outputs(str(tmp_path / "plain"), R.NAMES)
    assert R.read_outputs(str(tmp_path / "odd"), R.NAMES) == want
    exp = R.py_filter(texts, wl_bytes, 14, 77, 0.5, True)
    assert all(want[n] == exp[n] for n in R.NAMES) and 0 < len(R.records(want["R1"])) < 3000


def test_extract(tmp_path):
    c = TagCase(n=3000, n_cb=30, seed=1)
    c.write(str(tmp_path / "in.bam"))
    os.makedirs(tmp_path / "plain"), os.makedirs(tmp_path / "odd")
    so = _run("extract", ["-b", tmp_path / "in.bam", "-t", "xf", "-T", "1"], tmp_path / "plain")
    so2 = _run("extract", ["--bam=%s" % (tmp_path / "in.bam"), "-txf", "--type=0x1", "stray", "-T", "0"], tmp_path / "odd")
    assert so2 == so
    want = (tmp_path / "plain" / "tag_summary.csv").read_bytes()
    assert (tmp_path / "odd" / "tag_summary.csv").read_bytes() == want
    rows = dict(r.split(b",") for r in want.split(b"\n")[:-1])
    assert rows and sum(int(v) for v in rows.values()) == c.n and all(k.lstrip(b"-").isdigit() for k in rows)       # printed as "%d": the integer form


def test_cap(tmp_path):
    bam, b, f, lf, pf = TP._write(tmp_path, LH.labcase())
    so = _run("cap", ["-b", bam, "-a", b, "-f", f, "-o", tmp_path / "plain", "-c", "0.5", "-n", "3,8", "-s", "7", "--reps", "2", "--genes", "--cells",
                      "--labels", lf, "--markers", "3"], tmp_path)
    so2 = _run("cap", ["--bam=%s" % bam, "-a%s" % b, "--feature", f, "--out=%s" % (tmp_path / "odd"), "--cell=0.5", "--reads", "3,8", "-s0x7", "--reps=2", "--genes",
                       "--cells", "--labels=%s" % lf, "--markers=3", "-d", "x", "stray", "--fidelity", "-s", "1"], tmp_path)
    assert so2 == so
    want = _content(tmp_path / "plain")
    assert _content(tmp_path / "odd") == want
    points = {os.path.dirname(n) for n in want if os.path.basename(n) == "matrix.mtx.gz"}
    assert len(points) == 4 and {p.rpartition("_")[2] for p in points} == {"s7", "s8"}
    assert {"cap.tsv", "cap_reps.tsv", "cap_genes.tsv", "cap_cells.tsv", "cap_labels.tsv", "cap_markers.tsv"} <= set(want) and "cap_fidelity.tsv" not in want
