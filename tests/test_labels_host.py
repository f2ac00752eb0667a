"""--labels on the host: the loader of the labels file (format, label ids, every refusal with its line number), the host twin
fastf_label_votes against labels_ref on hand-built neighbour sets, the formatters of the four files, the refusals and spellings of the
interface, and the census of the fixtures test_gpu_labels shares."""
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, level, sweep, synth
from oracle import oracle as O
import labels_ref as LR
import neighbors_ref as N
from sweep_ref import parse_matrix

NONE = 0xFFFFFFFF


# ---- the loader ----
def _files(tmp_path, text, barcodes=("AAA-1", "CCC-1", "GGG-1", "TTT-1")):
    b, lf = tmp_path / "b.tsv", tmp_path / "labels.tsv"
    b.write_bytes(b"".join(x.encode() + b"\n" for x in barcodes))
    lf.write_bytes(text if isinstance(text, bytes) else text.encode())
    return lf, b


def test_header_cr_na_and_the_ids_in_bytewise_order(tmp_path):
    body = "GGG-1\tT cell\r\nAAA-1\tB\n\nCCC-1\tNA\nZZZ-9\tT\nTTT-1\tT\nYYY-9\tNA\n"
    for head in ("barcode\tcluster\n", ""):
        lf, b = _files(tmp_path, head + body)
        t = sweep.Labels(lf, b)
        assert t.n_labels == 3 and t.names == [b"NA", b"B", b"T", b"T cell"]      # "T" is a prefix of "T cell": the shorter first
        assert (t.known, t.unknown) == (4, 2)
        assert [t.id(x) for x in ("AAA-1", "CCC-1", "GGG-1", "TTT-1", "ZZZ-9", "nobody")] == [1, 0, 3, 2, 2, 0]
        assert list(t.assign(["TTT-1", "AAA-1", "CCC-1", "missing"])) == [2, 1, 0, 0]
        t.close()
    # a first field that is not exactly `barcode` is data; file order does not matter; bytes above 127 sort after ASCII
    lf, b = _files(tmp_path, "barcodes\tx\nTTT-1\t\xc3\xa9\nGGG-1\tz\nAAA-1\tZ\n".encode("latin-1"))
    t = sweep.Labels(lf, b)
    assert t.names == [b"NA", b"Z", b"x", b"z", b"\xc3\xa9"] and t.unknown == 1 and [t.id(x) for x in ("AAA-1", "GGG-1", "TTT-1", "barcodes")] == [1, 3, 4, 2]
    names, ids = LR.label_ids([("TTT-1", "T"), ("AAA-1", "B"), ("GGG-1", "T cell"), ("CCC-1", "NA")])
    assert names == ["NA", "B", "T", "T cell"] and ids == {"TTT-1": 2, "AAA-1": 1, "GGG-1": 3, "CCC-1": 0}


def test_255_labels_pass_and_256_are_refused(tmp_path):
    bars = ["B%04d" % i for i in range(300)]
    lf, b = _files(tmp_path, "".join("%s\tL%03d\n" % (x, 254 - i if i < 255 else i % 255) for i, x in enumerate(bars)), bars)
    t = sweep.Labels(lf, b)
    assert t.n_labels == 255 and t.names[1] == b"L000" and t.names[255] == b"L254" and t.id("B0000") == 255 and t.id("B0254") == 1
    lf, b = _files(tmp_path, "".join("%s\tL%03d\n" % (x, i) for i, x in enumerate(bars)), bars)
    with pytest.raises(F.FastfError, match=r"labels\.tsv: line 256 brings distinct label 256, at most 255"):
        sweep.Labels(lf, b)


@pytest.mark.parametrize("text,message", [
    ("AAA-1\tx\nCCC-1\n", r"line 2 has 1 fields"),
    ("AAA-1\tx\n\nCCC-1\ty\tz\n", r"line 3 has 3 fields"),
    ("barcode\tlabel\nAAA-1\t\n", r"line 2: the label is empty"),
    ("AAA-1\t" + "x" * 64 + "\n", r"line 1: the label has 64 bytes, at most 63"),
    ("AAA-1\tx\nCCC-1\ty\r\nAAA-1\tx\n", r"line 3 names barcode AAA-1 again \(first on line 1\)"),
    ("QQQ-1\tx\nRRR-1\tNA\n", r"no line names a barcode of "),
    (b"\x1f\x8b\x08\x00rest", r"starts with the gzip magic"),
])
def test_the_refusals_of_the_loader(tmp_path, text, message):
    lf, b = _files(tmp_path, text)
    with pytest.raises(F.FastfError, match=r"labels.*labels\.tsv.*" + message):
        sweep.Labels(lf, b)


def test_a_label_of_63_bytes_and_a_missing_file(tmp_path):
    lf, b = _files(tmp_path, "AAA-1\t" + "x" * 63 + "\n")
    assert sweep.Labels(lf, b).names[1] == b"x" * 63
    with pytest.raises(F.FastfError, match=r"labels file: .*nothing\.tsv does not exist"):
        sweep.Labels(tmp_path / "nothing.tsv", b)


# ---- the vote fixtures (shared with test_gpu_labels) ----
def _slots(sets, k):
    idx = np.full((len(sets), k), NONE, np.uint32)
    for i, s in enumerate(sets):
        idx[i, :len(s)] = s
    return idx, np.array([len(s) for s in sets], np.uint32)


def hand_fixture(name):
    """(idx, cnt, lab, k, n_labels) of a hand-built case"""
    if name == "two_way_tie":        # cell 0: two votes for 3 and two for 2 — 2 wins, a reversed tie rule gives 3; cell 1: 3 alone
        lab = [1, 3, 3, 2, 2, 3]
        sets = [[1, 2, 3, 4], [2, 5], [0], [], [0, 3], [1]]
        k, L = 4, 3
    elif name == "three_way_tie":    # cell 0: one vote each for 4, 2 and 3 — 2; cell 5: 4 and 3 — 3
        lab = [1, 4, 2, 3, 0, 1]
        sets = [[1, 2, 3], [0, 5], [], [4], [0], [1, 3, 4]]
        k, L = 5, 4
    elif name == "own_label_0":      # cells 0 and 3 are unlabelled: predicted all the same, same == 0, no conf entry
        lab = [0, 2, 2, 0, 1]
        sets = [[1, 2, 4], [0, 3], [1], [4], [0, 3]]
        k, L = 3, 2
    elif name == "unlabelled_neighbours":    # cell 0 has neighbours, none of them labelled: pred 0, labelled 0, conf[0][0]
        lab = [1, 0, 0, 2]
        sets = [[1, 2], [0, 3], [3], [0]]
        k, L = 2, 2
    elif name == "cnt_0":
        lab = [1, 2, 1]
        sets = [[], [], []]
        k, L = 15, 2
    elif name == "k_1":
        lab = [1, 2, 2, 0]
        sets = [[1], [0], [3], []]
        k, L = 1, 2
    elif name == "all_unlabelled":
        lab = [0] * 7
        sets = [[(i + 1) % 7, (i + 2) % 7] for i in range(7)]
        k, L = 15, 3
    else:
        raise KeyError(name)
    idx, cnt = _slots(sets, k)
    return idx, cnt, np.array(lab, np.uint8), k, L


HAND = ("two_way_tie", "three_way_tie", "own_label_0", "unlabelled_neighbours", "cnt_0", "k_1", "all_unlabelled")
HAND_PRED = {"two_way_tie": [2, 3, 1, 0, 1, 3], "three_way_tie": [2, 1, 0, 0, 1, 3], "own_label_0": [2, 0, 2, 1, 0], "unlabelled_neighbours": [0, 1, 2, 1],
             "cnt_0": [0, 0, 0], "k_1": [2, 1, 0, 0], "all_unlabelled": [0] * 7}


def random_fixture(n, k, n_labels, seed, p_unlabelled=0.2):
    """n cells with 0 .. min(k, n - 1) distinct neighbours each (ascending, never the cell itself), labels 0 .. n_labels"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(1, n_labels + 1, size=n).astype(np.uint8)
    if n_labels <= 2 and n > 1:
        lab[:] = 1 + (np.arange(n) * 7 // 3) % n_labels
    lab[rng.random(n) < p_unlabelled] = 0
    sets = []
    for i in range(n):
        c = 0 if i == 1 else int(rng.integers(0, min(k, n - 1) + 1)) if i % 5 else min(k, n - 1)      # (cell 1 has no neighbour: pred 0)
        others = np.delete(np.arange(n), i)
        sets.append(sorted(int(v) for v in rng.choice(others, size=c, replace=False)) if c else [])
    idx, cnt = _slots(sets, k)
    return idx, cnt, lab, k, n_labels


def overwritten_pads(fx):
    """the same sets, every pad slot overwritten with the index of a cell of another label than the cell's first neighbour has (where
    there is one): a reader that goes past cnt changes the vote"""
    idx, cnt, lab, k, L = fx
    idx = idx.copy()
    n = len(cnt)
    for i in range(n):
        first = lab[idx[i, 0]] if cnt[i] else 0
        other = [j for j in range(n) if lab[j] and lab[j] != first]
        if other:
            idx[i, cnt[i]:] = other[i % len(other)]
    return idx, cnt, lab, k, L


def pads_fixture():
    """cell i: one neighbour of label 1, then 14 pad slots — overwritten, they all name a cell of label 2"""
    lab = np.array([1, 1, 2, 2, 1], np.uint8)
    idx, cnt = _slots([[1], [0], [0], [1], [0]], 15)
    return overwritten_pads((idx, cnt, lab, 15, 2))


def reference(fx):
    idx, cnt, lab, k, L = fx
    return LR.votes(LR.sets_of_slots(idx, cnt), [int(v) for v in lab], L)


def check_against_reference(got, fx):
    pred, same, labelled, conf = reference(fx)
    assert [int(v) for v in got[0]] == pred and [int(v) for v in got[1]] == same and [int(v) for v in got[2]] == labelled
    assert np.asarray(got[3]).reshape(fx[4], fx[4] + 1).tolist() == conf


@pytest.mark.parametrize("name", HAND)
def test_the_host_twin_on_the_hand_built_sets(name):
    fx = hand_fixture(name)
    got = sweep.label_votes(*fx)
    check_against_reference(got, fx)
    assert [int(v) for v in got[0]] == HAND_PRED[name]
    check_against_reference(sweep.label_votes(*overwritten_pads(fx)), fx)


def test_the_tie_rule_and_the_pads_decide():
    fx = hand_fixture("two_way_tie")
    pred, same, labelled, conf = reference(fx)
    assert pred[0] == 2 and labelled[0] == 4 and same[0] == 0 and conf[0] == [0, 0, 1, 0]
    fx = hand_fixture("unlabelled_neighbours")
    assert reference(fx)[3][0] == [1, 0, 0]
    fx = pads_fixture()
    got = sweep.label_votes(*fx)
    assert [int(v) for v in got[0]] == [1, 1, 1, 1, 1] and [int(v) for v in got[2]] == [1] * 5
    # read past cnt, the pads would outvote the one neighbour
    read_all = LR.votes([[int(v) for v in row] for row in fx[0]], [int(v) for v in fx[2]], 2)
    assert read_all[0] == [2, 2, 2, 2, 2]


@pytest.mark.parametrize("n,k,L", [(17, 15, 3), (65, 33, 5), (40, 64, 255), (30, 1, 1), (257, 16, 128)])
def test_the_host_twin_on_random_sets(n, k, L):
    fx = random_fixture(n, k, L, seed=n + k)
    check_against_reference(sweep.label_votes(*fx), fx)
    check_against_reference(sweep.label_votes(*overwritten_pads(fx)), fx)


def test_the_twin_refuses_k_and_labels_out_of_range():
    idx, cnt, lab, k, L = hand_fixture("k_1")
    for bad in (0, 65):
        with pytest.raises(F.FastfError, match="from 1 to 64"):
            _lib.check(_lib.lib().fastf_label_votes(idx.ctypes.data, cnt.ctypes.data, lab.ctypes.data, 4, bad, 2, lab.ctypes.data, lab.ctypes.data, lab.ctypes.data, idx.ctypes.data))
    with pytest.raises(F.FastfError, match="256 labels, at most 255"):
        _lib.check(_lib.lib().fastf_label_votes(idx.ctypes.data, cnt.ctypes.data, lab.ctypes.data, 4, 1, 256, lab.ctypes.data, lab.ctypes.data, lab.ctypes.data, idx.ctypes.data))


# ---- the rows ----
def test_headers_rows_and_the_na_rules():
    assert sweep.labels_header().rstrip("\n").split("\t") == list(sweep.POINT_LABELS_COLUMNS)
    for verb, mod in (("sweep", sweep), ("cap", cap), ("level", level)):
        assert sweep.labels_header(verb).rstrip("\n").split("\t") == list(mod.LABELS_COLUMNS)
        assert sweep.labels_header(verb, classes=True).rstrip("\n").split("\t") == list(mod.LABEL_CLASSES_COLUMNS)
        assert mod.LABELS_COLUMNS[2:] == sweep.LABELS_TAIL_COLUMNS and mod.LABEL_CLASSES_COLUMNS[2:] == sweep.LABEL_CLASSES_TAIL_COLUMNS
    assert cap.LABELS_COLUMNS[1] == "reads_per_cell" and level.LABELS_COLUMNS[1] == "umi_cap" and sweep.LABEL_CLASSES_COLUMNS[1] == "rate_depth"
    fx = random_fixture(40, 15, 3, seed=3)
    lab = [int(v) for v in fx[2]]
    full = reference(fx)
    point = reference(random_fixture(40, 15, 3, seed=4)[:2] + fx[2:])
    names = ["NA", "B", "T", "T cell"]
    bcs = ["BC%02d" % i for i in range(40)]
    for i, want in enumerate(LR.cell_rows(bcs, names, lab, full, point)):
        assert sweep.labels_row(bcs[i], names[lab[i]], names[full[0][i]], names[point[0][i]], full[1][i], full[2][i], point[1][i], point[2][i]) == "\t".join(want) + "\n"
    rows = LR.confusion_rows(names, lab, point[3])
    assert sweep.label_confusion_header(names) == "label\tcells\tNA\tB\tT\tT cell\n" == "\t".join(rows[0]) + "\n"
    for a in (1, 2, 3):
        assert sweep.label_confusion_row(names[a], lab.count(a), point[3][a - 1]) == "\t".join(rows[a]) + "\n"
    arrays = (fx[2], full[0], point[0], full[1], full[2], point[1], point[2], full[3], point[3])
    assert sweep.labels_summary_row(0.5, 0.1, 926, 15, 3, *arrays).rstrip("\n").split("\t") == LR.summary_fields(["0.500", "0.100"], 926, 15, 3, lab, full, point)
    assert sweep.labels_summary_row(0.5, 0, 7, 15, 3, *arrays, list_value=20).split("\t")[:3] == ["0.500", "20", "7"]
    want = LR.classes_fields(["1.000", "300"], 5, names, lab, full, point)
    for a in (1, 2, 3):
        assert sweep.label_classes_row(1, 0, 5, names[a], a, 3, fx[2], full[3], point[3], list_value=300).rstrip("\n").split("\t") == want[a - 1]
    # every ratio is NA on a zero denominator: no labelled cell at all, and kept with agree_full == 0
    z8, zc = np.zeros(4, np.uint8), np.zeros(6, np.uint32)
    assert sweep.labels_summary_row(1, 1, 1, 15, 2, z8, z8, z8, z8, z8, z8, z8, zc, zc) == "1.000\t1.000\t1\t4\t15\t2\t0\t0\t0\tNA\tNA\tNA\tNA\tNA\n"
    lab2 = np.array([1, 2, 1, 0], np.uint8)
    wrong = reference((_slots([[1], [0], [1], [0]], 1)[0], np.ones(4, np.uint32), lab2, 1, 2))          # every labelled cell is predicted the other label
    assert wrong[0] == [2, 1, 2, 1] and wrong[3] == [[0, 0, 2], [0, 1, 0]]
    f = sweep.labels_summary_row(1, 1, 1, 1, 2, lab2, wrong[0], wrong[0], wrong[1], wrong[2], wrong[1], wrong[2], wrong[3], wrong[3]).rstrip("\n").split("\t")
    assert f[6:] == ["3", "0", "0", "0.000000", "0.000000", "NA", "0.000000", "0.000000"]
    assert f == LR.summary_fields(["1.000", "1.000"], 1, 1, 2, [1, 2, 1, 0], wrong, wrong)


# ---- the interface ----
def test_the_entry_points_the_spellings_and_the_refusals(tmp_path):
    one, p_one = sweep._floats([1])
    caps = np.array([5], np.uint64)
    seeds = caps.astype(np.uint32)
    L = _lib.lib()
    for name in ("fastf_sweep_labels", "fastf_cap_labels", "fastf_level_labels", "fastf_dev_label_votes", "fastf_label_votes", "fastf_labels_load"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name)
    assert "label_votes_kernel" in L.fastf_kernel_names().decode().split(",")
    calls = (lambda fl, ns: L.fastf_sweep_labels(b"x", b"y", b"b", b"f", p_one, 1, p_one, 1, seeds.ctypes.data, ns, fl, 926, None),
             lambda fl, ns: L.fastf_cap_labels(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, seeds.ctypes.data, ns, fl, 926, None),
             lambda fl, ns: L.fastf_level_labels(b"x", b"y", b"b", b"f", p_one, 1, caps.ctypes.data, 1, seeds.ctypes.data, ns, fl, 926, None))
    for call in calls:                                      # labels_path == NULL: exactly the old calls, plain and replicate
        for ns in (0, 1):
            with pytest.raises(F.FastfError, match="does not exist"):
                _lib.check(call(512 | 128 | 32 | 8 | 2 | 1, ns))
            for flags in (4, 16, 64, 256, 1024, 2048):      # no new bit
                with pytest.raises(F.FastfError, match="unknown flags"):
                    _lib.check(call(flags, ns))
    bt, ft, bar, genes = synth.make_lists(5, 3)
    fl, xf, cb, gx, ub = synth.make_records(20, bar, genes)
    bam, b, f, lf = tmp_path / "x.bam", tmp_path / "b.tsv", tmp_path / "f.tsv", tmp_path / "labels.tsv"
    synth.write_bam(str(bam), fl, xf, cb, gx, ub)
    b.write_bytes(bt); f.write_bytes(ft)
    lf.write_bytes(b"".join(x + b"\tT\n" for x in bar.tolist()))
    with pytest.raises(F.FastfError, match="bam file: .* does not exist"):
        sweep.sweep(tmp_path / "no.bam", tmp_path / "o", b, f, [1], [1], labels=lf)
    several = dict(os.environ, FASTF_DEVICES="0,1")
    for k, (verb, extra) in enumerate([("sweep", ["-r", "0.5"]), ("cap", ["-n", "5"]), ("level", ["-m", "5"])]):
        out = tmp_path / ("out%d" % k)
        base = [_lib.cli_path(), verb, "-o", str(out), "-a", str(b), "-f", str(f), "-b", str(bam)] + extra
        for more in ([], ["--neighbors", "--fidelity"], ["--seeds", "1,2"]):
            r = subprocess.run(base + ["--labels", str(lf)] + more, capture_output=True, text=True, timeout=60, env=several)
            assert r.returncode == 1 and "several devices" in r.stderr, r.stderr
            assert "%s: --labels needs the resident form" % verb in r.stderr
            assert not out.exists()                         # refused before the output directory is made
        for text, message in (("nobody\tT\n", "no line names a barcode"), ("%s\tT\textra\n" % bar[0].decode(), "line 1 has 3 fields")):
            bad = tmp_path / "bad.tsv"
            bad.write_text(text)
            r = subprocess.run(base + ["--labels=" + str(bad)], capture_output=True, text=True, timeout=60)
            assert r.returncode == 1 and message in r.stderr and "bad.tsv" in r.stderr and not out.exists(), r.stderr
        r = subprocess.run(base + ["--labels", str(tmp_path / "none.tsv")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "labels file:" in r.stderr and "does not exist" in r.stderr and not out.exists()
        r = subprocess.run([_lib.cli_path(), verb, "--help"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "--labels=<file>" in r.stdout and "%s_labels.tsv" % verb in r.stdout and "%s_label_classes.tsv" % verb in r.stdout
        for opt in (["-L", str(lf)], ["--label", str(lf)], ["--label=" + str(lf)]):    # the long form alone
            r = subprocess.run([_lib.cli_path(), verb] + opt + ["-o", str(out)], capture_output=True, text=True, timeout=60)
            assert r.returncode == 1 and "unknown option" in r.stderr
        r = subprocess.run([_lib.cli_path(), verb, "-o", str(out), "--labels"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "option `--labels` requires a value" in r.stderr and not out.exists()
    os.environ["FASTF_DEVICES"] = "0,1"
    try:
        with pytest.raises(F.FastfError, match="sweep: --labels needs the resident form.*several devices"):
            sweep.sweep(bam, tmp_path / "o", b, f, [1], [1], labels=lf)
        with pytest.raises(F.FastfError, match="cap: --labels needs the resident form.*several devices"):
            cap.cap_reps(bam, tmp_path / "o", b, f, [1], [5], [1, 2], labels=lf)
        with pytest.raises(F.FastfError, match="level: --labels needs the resident form.*several devices"):
            level.level(bam, tmp_path / "o", b, f, [1], [5], labels=lf, neighbors=True)
    finally:
        del os.environ["FASTF_DEVICES"]
    assert not (tmp_path / "o").exists()


# ---- the synthetic BAM the commands run on (shared with test_gpu_labels) ----
class LabCase:
    """600 records of 60 barcodes x 45 genes: a cell of type t draws four of five reads from the t-th block of 15 genes.  The labels
    file names the types by blocks of cells, leaves some cells out, calls some NA, mislabels a few, and names barcodes nobody lists"""
    TYPES = ("T cell", "B", "T")
    seed = 926

    def __init__(self):
        self.bt, self.ft, self.bar, self.genes = synth.make_lists(60, 45, seed=77)
        n = 600
        fl, xf, cb, gx, ub = synth.make_records(n, self.bar, self.genes, seed=5, umi_len=10)
        rng = np.random.default_rng(11)
        cell = rng.integers(0, 60, size=n)
        own = rng.random(n) < 0.8
        gene = np.where(own, (cell % 3) * 15 + rng.integers(0, 15, size=n), rng.integers(0, 45, size=n))
        self.flags, self.xf = fl, np.full(n, 25, np.int32)
        self.cb, self.gx, self.ub = synth.as_cstr(self.bar[cell].copy()), synth.as_cstr(self.genes[gene].copy()), synth.as_cstr(ub)
        lines = ["barcode\ttype"]
        for i, bc in enumerate(self.bar.tolist()):
            if i % 10 == 9:
                continue                                    # no line: unlabelled
            t = "NA" if i % 10 == 8 else self.TYPES[(i + (1 if i % 13 == 0 else 0)) % 3]
            lines.append("%s\t%s" % (bc.decode(), t))
        lines += ["NOBODY-1\tT", "NOBODY-2\tNA"]
        self.labels_text = ("\n".join(lines[:1] + lines[:0:-1]) + "\n").encode()      # (the rows in reverse file order)
        self.pairs = [tuple(ln.split("\t")) for ln in lines[1:]]
        self._matrix = {}

    def matrix(self, rate_cell, rate_depth, seed=926):
        """(rows, barcodes) of the oracle's matrix at a point; rate_depth 1: the full-depth rows of the pair"""
        key = (float(rate_cell), float(rate_depth), seed)
        if key not in self._matrix:
            ora = O.run_bam2db(self.bt, self.ft, self.flags, self.xf, self.cb, self.gx, self.ub, float(np.float32(rate_cell)), float(np.float32(rate_depth)),
                               seed, b"x.bam", False)
            _, _, _, f, c, v = parse_matrix(ora["matrix"])
            self._matrix[key] = ((f, c, v), ora["barcodes"].decode().split("\n")[:-1])
        return self._matrix[key]


_LABCASE = []


def labcase():
    if not _LABCASE:
        _LABCASE.append(LabCase())
    return _LABCASE[0]


def reference_point(case, full_rows, point_rows, barcodes, n_features=45, k=15):
    """(names, lab, full, point) by the reference alone: A from the full rows, both neighbour sets, both votes"""
    names, ids = LR.label_ids(case.pairs)
    lab = [ids.get(bc, 0) for bc in barcodes]
    n = len(barcodes)
    A = N.hvg_of_rows(full_rows, n, n_features)
    full = LR.votes(N.neighbor_sets(full_rows, n, A, k)[0], lab, len(names) - 1)
    point = LR.votes(N.neighbor_sets(point_rows, n, A, k)[0], lab, len(names) - 1)
    return names, lab, full, point


def test_census_of_the_shared_fixtures():
    case = labcase()
    full_rows, barcodes = case.matrix(1, 1)
    point_rows, barcodes2 = case.matrix(1, 0.1)
    assert barcodes == barcodes2 and len(barcodes) == 60
    names, lab, full, point = reference_point(case, full_rows, point_rows, barcodes)
    assert names == ["NA", "B", "T", "T cell"]
    ids = [i for i, x in enumerate(lab) if x]
    assert 40 <= len(ids) < 60
    assert sum(1 for i in ids if full[2][i] > 0) * 2 >= len(ids)
    for m in (full, point):
        assert any(m[0][i] == lab[i] for i in ids) and any(m[0][i] != lab[i] for i in ids)
    assert any(point[3][a][b] for a in range(3) for b in range(1, 4) if b != a + 1)
    assert 0 in point[0] and point != full
    # the device fixtures: every group size, both sides of the LDS limit, ties and empty sets among them
    for n, k, L in ((1000, 15, 30), (257, 33, 201), (65, 64, 202)):
        fx = random_fixture(n, k, L, seed=1)
        pred, same, labelled, conf = reference(fx)
        assert 0 in pred and int(fx[1].max()) == min(k, n - 1) and 0 in fx[1] and any(conf[a][b] for a in range(L) for b in range(L + 1) if b != a + 1)
