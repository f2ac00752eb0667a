"""fastf_amd — MI355X-native bam2db UMI-counting engine (drop-in for fastF's bam2db path).

The product is the C-ABI shared library ``fastf_amd/lib/libfastf_amd.so`` (hand-written
HIP kernels for gfx950 + the C host side, see include/fastf_amd.h).  This package is the
thin Python host mirror used by the tests, bench.py and the multi-GPU launcher; torch is
only plumbing here (device memory, streams, torch.distributed over RCCL).
"""
from ._lib import build, lib, lib_path, FastfError  # noqa: F401
from .engine import Engine, Lists, PinnedBatch, pack_records, draw_threshold, mt_draws  # noqa: F401
from .fastq import freq, freq_text, filter, filter_draws, filter_rand_at, fqcap, fqcap_rate, fqcells, fqcells_call  # noqa: F401
from . import cap  # noqa: F401  (the module: cap.cap() is the command, as sweep.sweep() is)
from . import level  # noqa: F401  (the module: level.level() is the command)

__all__ = ["build", "lib", "lib_path", "FastfError", "Engine", "Lists", "PinnedBatch", "pack_records",
           "draw_threshold", "mt_draws", "freq", "freq_text", "filter", "filter_draws", "filter_rand_at", "fqcap", "fqcap_rate", "fqcells", "fqcells_call", "cap", "level"]
