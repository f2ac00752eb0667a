"""The three ways into a grid run on the GPU — the command, the Python function and the most general entry point called directly —
with every option on: each leaves the same files with the same content, for one seed and for a replicate run."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from fastf_amd import _lib, sweep
import test_gpu_labels as TL
import test_gpu_ptime as TP
import test_labels_host as LH

pytestmark = pytest.mark.gpu

FLAGS = sweep.GENES | sweep.CELLS | sweep.FIDELITY | sweep.GENE_FIDELITY | sweep.NEIGHBORS | sweep.COEXPRESSION
RATES = [0.5]


def _content(root):
    """every file under root by its relative name, the gzipped ones decompressed"""
    return {n: gzip.decompress(v) if n.endswith(".gz") else v for n, v in TL._tree(root).items()}


@pytest.mark.parametrize("seeds", [None, [7, 8]], ids=["seed", "seeds"])
@pytest.mark.parametrize("verb", ["sweep", "cap", "level"])
def test_the_command_the_function_and_the_direct_call_leave_the_same_files(tmp_path, verb, seeds):
    bam, b, f, lf, pf = TP._write(tmp_path, LH.labcase())
    values = TL.GRID[verb]
    by_cli, by_python, by_call = tmp_path / "cli", tmp_path / "python", tmp_path / "call"
    r = subprocess.run(TL._args(verb, bam, b, f, by_cli, RATES, values) + (["-s", "7"] if seeds is None else ["--seeds", ",".join(str(x) for x in seeds)]) +
                       ["--genes", "--cells", "--fidelity", "--gene-fidelity", "--neighbors", "--coexpression", "--labels", str(lf), "--markers", "3", "--mapping",
                        "--pseudotime", str(pf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    opts = dict(genes=True, cells=True, fidelity=True, gene_fidelity=True, neighbors=True, coexpression=True, labels=lf, markers=3, mapping=True, pseudotime=pf)
    if seeds is None:
        TL.MOD[verb].__dict__[verb](bam, by_python, b, f, RATES, values, seed=7, **opts)
    else:
        TL.MOD[verb].__dict__[verb + "_reps"](bam, by_python, b, f, RATES, values, seeds, **opts)
    enc = lambda p: os.fspath(p).encode()  # noqa: E731
    rc, prc = sweep._floats(RATES)
    lv = np.ascontiguousarray(values, np.float32 if verb == "sweep" else np.uint64)
    sd = np.ascontiguousarray(seeds or [], np.uint32)
    _lib.check(getattr(_lib.lib(), "fastf_%s_pseudotime" % verb)(
        enc(bam), enc(by_call), enc(b), enc(f), prc, len(rc), lv.ctypes.data_as(C.POINTER(C.c_float)) if verb == "sweep" else lv.ctypes.data, len(lv),
        sd.ctypes.data if seeds else None, len(sd), FLAGS, 7 if seeds is None else 0, enc(lf), 3, 1, enc(pf)))
    want = _content(by_cli)
    stems = ["", "_genes", "_cells", "_fidelity", "_gene_fidelity", "_neighbors", "_coexpr", "_labels", "_label_classes", "_markers", "_mapping", "_pseudotime"]
    assert {"%s%s.tsv" % (verb, s) for s in stems} <= set(want) and ("%s_reps.tsv" % verb in want) == (seeds is not None)
    points = {os.path.dirname(n) for n in want if os.path.basename(n) == "pseudotime.tsv.gz"}
    assert len(points) == len(RATES) * len(values) * len(seeds or [7]) and all(p.endswith("_s7") or p.endswith("_s8") for p in points) == (seeds is not None)
    for other in (by_python, by_call):
        got = _content(other)
        assert sorted(got) == sorted(want)
        assert [n for n in want if got[n] != want[n]] == []
