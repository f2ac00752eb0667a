"""--coexpression without a device: the option of the three commands (the long form alone, in the help text), the flag bit of the entry
points (4096 accepted, the unassigned bits 1024 and 2048 beside it refused), the refusal with several devices before the output directory
is made, and the exported names."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, level, sweep

VERBS = ("sweep", "cap", "level")


def _calls():
    L = _lib.lib()
    one = np.ones(1, np.float32)
    caps = np.array([5], np.uint64)
    p_one = one.ctypes.data_as(C.POINTER(C.c_float))
    keep = (one, caps)
    return {"sweep": lambda bam, out, fl: (keep, L.fastf_sweep(bam, out, b"b", b"f", p_one, 1, p_one, 1, 926, fl))[1],
            "cap": lambda bam, out, fl: (keep, L.fastf_cap(bam, out, b"b", b"f", p_one, 1, caps.ctypes.data, 1, 926, fl))[1],
            "level": lambda bam, out, fl: (keep, L.fastf_level(bam, out, b"b", b"f", p_one, 1, caps.ctypes.data, 1, 926, fl))[1]}


@pytest.mark.parametrize("verb", VERBS)
def test_the_option_is_the_long_form_alone_and_in_the_help(verb):
    r = subprocess.run([_lib.cli_path(), verb, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--coexpression" in r.stdout and "%s_coexpr.tsv" % verb in r.stdout
    for bad in ("-X", "--coexpr", "--coexpressio"):
        r = subprocess.run([_lib.cli_path(), verb, bad], capture_output=True, text=True)
        assert r.returncode != 0 and "unknown option `%s`" % bad in r.stderr
    r = subprocess.run([_lib.cli_path(), verb, "--coexpression", "-b", "/nonexistent.bam", "-c", "1", {"sweep": "-r", "cap": "-n", "level": "-m"}[verb], "1"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "does not exist" in r.stderr and "unknown option" not in r.stderr


@pytest.mark.parametrize("verb", VERBS)
def test_flag_4096_is_accepted_and_the_unassigned_bits_are_refused(verb):
    call = _calls()[verb]
    assert sweep.COEXPRESSION == cap.COEXPRESSION == level.COEXPRESSION == 4096
    for flags in (4096, 4096 | 512 | 128 | 32 | 8 | 2 | 1):
        with pytest.raises(F.FastfError, match="does not exist"):
            _lib.check(call(b"x", b"y", flags))
    for flags in (4096 | 1024, 4096 | 2048, 8192):
        with pytest.raises(F.FastfError, match="unknown flags"):
            _lib.check(call(b"x", b"y", flags))


@pytest.mark.parametrize("verb", VERBS)
def test_several_devices_are_refused_by_name_before_the_directory_is_made(verb, tmp_path, monkeypatch):
    bam, out = tmp_path / "x.bam", tmp_path / "out"
    bam.write_bytes(b"")
    monkeypatch.setenv("FASTF_DEVICES", "0,1")
    with pytest.raises(F.FastfError, match="%s: --coexpression needs the resident form" % verb):
        _lib.check(_calls()[verb](str(bam).encode(), str(out).encode(), 4096))
    assert not out.exists()
    with pytest.raises(F.FastfError, match="%s: --neighbors needs the resident form" % verb):      # (the earlier option keeps its place in the order)
        _lib.check(_calls()[verb](str(bam).encode(), str(out).encode(), 4096 | 512))
    assert not out.exists()


def test_exported_names_and_the_python_mirror():
    L = _lib.lib()
    for name in ("fastf_coexpr_pad", "fastf_coexpr_work_bytes", "fastf_dev_coexpr_sums", "fastf_dev_coexpr_select"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name)
    for name in ("dev_coexpr_sums", "dev_coexpr_select"):
        assert hasattr(F.Engine, name)
    names = L.fastf_kernel_names().decode().split(",")
    assert {"coex_planes_kernel", "coex_gram_kernel", "coex_sums_kernel", "coex_var_kernel", "coex_select_kernel"} <= set(names)
    K_pad, n_pad, chunk = sweep.coexpression_pad(25_000, 2000)
    assert (K_pad, chunk) == (2016, sweep.COEXPRESSION_CHUNK) and n_pad % chunk == 0 and 25_000 <= n_pad < 25_024 + chunk
    assert sweep.coexpression_work_bytes(25_000, 2000, 2) == 2 * K_pad * n_pad
    for verb, mod in (("sweep", sweep), ("cap", cap), ("level", level)):
        assert sweep.coexpression_header(verb) == "\t".join(mod.COEXPRESSION_COLUMNS) + "\n"
