"""filter without a GPU: the host jump-ahead of glibc's rand() against libc's srand / rand, the reference's keep rule on edge
draws, and the command line's argument errors against the reference's own (oracle/_ref/fastF_refmain) plus our refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib

import filter_ref as R

OURS = _lib.cli_path()
libc = C.CDLL("libc.so.6")
libc.srand.argtypes = [C.c_uint]
libc.rand.restype = C.c_int


@pytest.mark.parametrize("seed", [0, 1, 926, 2 ** 31, 2 ** 32 - 1])
def test_jump_ahead_equals_libc(seed):
    offsets = [0, 30, 31, 344, 10 ** 6, 10 ** 7 + 3]
    libc.srand(seed)
    want, i = {}, 0
    rand = libc.rand
    for off in offsets:
        while i < off:
            rand()
            i += 1
        want[off] = rand()
        i += 1
    for off in offsets:
        assert F.filter_rand_at(seed, off) == want[off], off


def test_host_stream_equals_libc():
    libc.srand(926)
    want = np.array([libc.rand() for _ in range(100_000)], dtype=np.uint32)
    assert np.array_equal(F.filter_draws(926, 0, 100_000, device=False), want)
    assert np.array_equal(F.filter_draws(926, 4097, 5000, device=False), want[4097:9097])


@pytest.mark.parametrize("r", [2 ** 31 - 1, 2 ** 31 - 64, 2 ** 31 - 65, 2 ** 24 + 1, 0])
@pytest.mark.parametrize("rate", [0.0, 0.5, 1.0, 2.0, float(np.float32(2 ** 24 + 1) / np.float32(2 ** 31))])
def test_keep_predicate_on_edge_draws(r, rate):
    want = float(np.float32(r) / np.float32(2147483647)) < float(np.float32(rate))
    assert bool(_lib.lib().fastf_filter_draw_passes(r, rate)) == want
    assert R.draw_passes(r, rate) == want


def test_rate_one_does_not_keep_every_draw():
    assert not _lib.lib().fastf_filter_draw_passes(2 ** 31 - 64, 1.0)
    assert _lib.lib().fastf_filter_draw_passes(2 ** 31 - 65, 1.0)


def run(binary, args, cwd):
    return subprocess.run([binary, "filter"] + args, capture_output=True, text=True, cwd=cwd, timeout=120)


@pytest.mark.parametrize("args", [
    ["-w", "wl.txt"],                         # no -R
    ["-R", "r1.fq"],                          # neither -w nor -a
    [],
])
def test_argument_errors_match_reference(tmp_path, args):
    if not os.path.exists(R.REFMAIN):
        pytest.skip("oracle/_ref/fastF_refmain not built")
    (tmp_path / "r1.fq").write_bytes(b"@a\nACGT\n+\nIIII\n")
    (tmp_path / "wl.txt").write_bytes(b"ACGT\n")
    ours, ref = run(OURS, args, tmp_path), run(R.REFMAIN, args, tmp_path)
    assert ours.returncode == ref.returncode == 1
    assert ours.stdout == ref.stdout
    assert ours.stderr == ref.stderr


def test_refusals_without_gpu(tmp_path):
    (tmp_path / "r1.fq").write_bytes(b"@a\nACGT\n+\nIIII\n")
    (tmp_path / "wl.txt").write_bytes(b"ACGT\n")
    (tmp_path / "long.txt").write_bytes(b"ACGT\n" + b"A" * 99 + b"\n")
    p = run(OURS, ["-R", "r1.fq", "-a", "-l", "-3"], tmp_path)
    assert p.returncode == 1 and "negative" in p.stderr
    p = run(OURS, ["-R", "r1.fq", "-a", "-o", str(tmp_path / "missing_dir")], tmp_path)
    assert p.returncode == 1 and "missing_dir" in p.stderr
    p = run(OURS, ["-R", "r1.fq", "-w", "long.txt"], tmp_path)
    assert p.returncode == 1 and "long.txt" in p.stderr and "line 2" in p.stderr
    assert not (tmp_path / "R1.fastq.gz").exists()
    if os.getuid() != 0:
        ro = tmp_path / "ro"
        ro.mkdir()
        ro.chmod(0o500)
        p = run(OURS, ["-R", "r1.fq", "-a", "-o", str(ro)], tmp_path)
        ro.chmod(0o700)
        assert p.returncode == 1 and "ro" in p.stderr


def test_help_and_dispatch():
    r = subprocess.run([OURS, "filter", "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--whitelist" in r.stdout and "--allcells" in r.stdout
    r = subprocess.run([OURS, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "filter" in r.stdout


def test_library_exports_filter():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for sym in ("fastF", "cmd_filter", "fastf_filter", "fastf_filter_draws", "fastf_filter_rand_at"):
        assert sym in names, sym
    for sym in ("in", "get_row", "read_txt", "combine_string", "fq_src_open"):
        assert sym not in names, sym
