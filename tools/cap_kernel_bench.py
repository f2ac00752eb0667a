"""cap's two kernels on the resident BASELINE configs[2] shape (fastf_amd/workload.py: 200 M records, 50 000 x 36 601): wall clock
around the calls, and — run under `rocprofv3 --kernel-trace --stats -- python tools/cap_kernel_bench.py` — the per-kernel lines of
cell_hits_kernel and cell_decisions_kernel beside K1a (probe_cells_*) and draw_planes_kernel of the same trace.  Two engines over the
same records: the sampled half of the barcodes (-c 0.5: 25 000 cells, LDS counters) and all of them (-c 1: 50 000 cells, two ranges of
LDS counters; FASTF_CAP_LDS_RANGES=0 in the environment gives the general form: wave-aggregated global atomics).

    python tools/cap_kernel_bench.py --records 200000000 --cap 1000 --reps 5
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fastf_amd as F  # noqa: E402
from fastf_amd import cap, hostmem  # noqa: E402
from fastf_amd.workload import C3, SEGMENTS, SEED  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200_000_000)
    ap.add_argument("--cap", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    job = C3(a.records)
    parts = [job.segment_packed(s, dev) for s in range(SEGMENTS)]
    cb, gx, umi, meta = (torch.cat([p[k] for p in parts]) for k in range(4))
    del parts
    n = a.records

    def timed(fn):
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3)
        return "%.3f ms (min of %d: %s)" % (min(ms), a.reps, " ".join("%.3f" % x for x in ms))

    print("%d records resident" % n)
    for lists, label in ((job.lists, "-c 0.5"), (job.all_lists, "-c 1")):
        eng = F.Engine.from_lists(lists, seed=SEED, umi_max_bases=12)
        n_cells = len(lists.cell_keys)
        blk = torch.zeros(eng.block_bytes(n) // 8, dtype=torch.int64, device=dev)
        eng.dev_block_records(gx.data_ptr(), umi.data_ptr(), meta.data_ptr(), n, blk.data_ptr())
        d_H = torch.zeros(1, dtype=torch.int64, device=dev)
        t_k1a = timed(lambda: eng.dev_count_hits_blocked(cb.data_ptr(), n, blk.data_ptr(), d_H.data_ptr()))
        H = int(d_H.item())
        d_h = torch.zeros(n_cells, dtype=torch.int32, device=dev)
        t_hits = timed(lambda: eng.dev_cell_hits(n, blk.data_ptr(), d_h.data_ptr()))
        h = hostmem.to_host(d_h).view(np.uint32)
        assert int(h.astype(np.uint64).sum()) == H
        T = cap.thresholds(h, a.cap)
        d_T = hostmem.to_device(T, dev)
        plane = torch.zeros((H + 63) // 64 * 2 + 64, dtype=torch.int32, device=dev)
        t0 = time.perf_counter()
        eng.dev_cell_decisions(n, blk.data_ptr(), SEED, lists.mt_skip, H, d_T.data_ptr(), plane.data_ptr())
        t_first = (time.perf_counter() - t0) * 1e3
        t_dec = timed(lambda: eng.dev_cell_decisions(n, blk.data_ptr(), SEED, lists.mt_skip, H, d_T.data_ptr(), plane.data_ptr()))
        kept = int(np.unpackbits(hostmem.to_host(plane).view(np.uint8)).sum())
        t_planes = timed(lambda: eng.dev_mt_decisions_multi(SEED, lists.mt_skip, H, [F.draw_threshold(0.5)], plane.data_ptr(), (H + 63) // 64 * 2))
        sb = eng.cell_scratch_bytes
        print("%s: %d cells (%s), scratch %d bytes per record, H = %d hits, cap %d: %d cells capped, %d hits kept" %
              (label, n_cells, "LDS counters, %d range(s)" % -(-n_cells // 32768) if n_cells <= 8 * 32768 and os.environ.get("FASTF_CAP_LDS_RANGES") is None else "see FASTF_CAP_LDS_RANGES", sb, H, a.cap, int((h > a.cap).sum()), kept))
        print("  K1a (fastf_dev_count_hits_blocked: probe + tile scan)       %s" % t_k1a)
        print("  fastf_dev_cell_hits (memset + cell_hits_kernel)             %s   reads %d bytes" % (t_hits, n * sb))
        print("  fastf_dev_cell_decisions, first call (generator inside)     %.3f ms" % t_first)
        print("  fastf_dev_cell_decisions (memset + cell_decisions_kernel)   %s   reads %d + %d bytes" % (t_dec, n * sb, 4 * H))
        print("  fastf_dev_mt_decisions_multi, one plane (generator + draw_planes_kernel)   %s" % t_planes)
        eng.close()
        del blk, plane
    return 0


if __name__ == "__main__":
    sys.exit(main())
