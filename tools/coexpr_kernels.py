"""The device calls of --coexpression on one large matrix, for a kernel trace or a wall-clock comparison: --cells cells x --genes genes,
5 % of the entries non-zero, counts below 2^7 (one plane) or below 2^14 (two planes, --planes 2).  fastf_dev_coexpr_sums (the gene-major
planes, the Gram kernel in the form FASTF_COEXPR_MFMA selects with the chunk FASTF_COEXPR_CHUNK leaves, the per-gene sums) and
fastf_dev_coexpr_select, each timed by a host clock around a device synchronise, --repeat times after one warm-up call; then
fastf_dev_neighbors_shared of the sets with themselves, which must give the counts back.  --host also runs the host twin
fastf_coexpr_from_coo on the same rows and compares D, S and the sets.

    rocprofv3 --kernel-trace --stats --output-format csv -d out -o cx -- python tools/coexpr_kernels.py --cells 25000 --planes 1
    FASTF_COEXPR_MFMA=0 python tools/coexpr_kernels.py --cells 25000 --planes 2 --host

The integer rate printed for the sums counts the multiply-adds of the tiles the Gram kernel computes: 2 * 32 * 32 * tiles * n32 * planes^2
operations, tiles = T (T + 1) / 2 of the T = K_pad / 32 rows of tiles."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import fastf_amd as F
from fastf_amd import hostmem, sweep
ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=25_000)
ap.add_argument("--genes", type=int, default=2000)
ap.add_argument("--planes", type=int, default=1)
ap.add_argument("--k", type=int, default=15)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--host", action="store_true")
a = ap.parse_args()
n, K, k = a.cells, a.genes, a.k
e = F.Engine(np.arange(1, 101, dtype=np.uint64) | (np.uint64(1) << np.uint64(62)), np.arange(1, 51, dtype=np.uint64) | (np.uint64(2) << np.uint64(62)), umi_max_bases=12)
g = torch.Generator(device="cuda"); g.manual_seed(1)
per = K // 20                                              # 5 % of the genes per cell, one in every stride of 20
cell = torch.arange(1, n + 1, device="cuda", dtype=torch.int32).repeat_interleave(per)
feat = (torch.arange(per, device="cuda", dtype=torch.int32) * 20).repeat(n) + torch.randint(1, 21, (n * per,), device="cuda", dtype=torch.int32, generator=g)
cnt = torch.randint(1, 100 if a.planes == 1 else 16000, (n * per,), device="cuda", dtype=torch.int32, generator=g)
d_n = torch.tensor([n * per], dtype=torch.int64, device="cuda")
sm = torch.from_numpy(sweep.neighbors_slot_map(np.arange(K), K).view(np.int16)).cuda()
p = lambda t: t.data_ptr()
P = e.dev_neighbor_planes(p(feat), p(cell), p(cnt), p(d_n), p(sm), K, n, K)
assert P == a.planes
K_pad, n_pad, chunk = sweep.coexpression_pad(n, K)
work = torch.empty(sweep.coexpression_work_bytes(n, K, P), dtype=torch.uint8, device="cuda")
D = torch.zeros(K * K, dtype=torch.int64, device="cuda")
S = torch.zeros(K, dtype=torch.int64, device="cuda")
idx = torch.zeros(K * k, dtype=torch.int32, device="cuda")
cn, sh = torch.zeros(K, dtype=torch.int32, device="cuda"), torch.zeros(K, dtype=torch.int32, device="cuda")


def timed(fn):
    fn(); torch.cuda.synchronize()                          # (warm-up: the code objects are loaded)
    ts = []
    for _ in range(a.repeat):
        t = time.time(); fn(); torch.cuda.synchronize(); ts.append(time.time() - t)
    return min(ts), sorted(ts)[len(ts) // 2]


t_sums = timed(lambda: e.dev_coexpr_sums(p(feat), p(cell), p(cnt), p(d_n), p(sm), K, n, K, P, p(work), work.numel(), p(D), p(S)))
t_sel = timed(lambda: e.dev_coexpr_select(p(D), p(S), n, K, k, p(idx), p(cn)))
e.dev_neighbors_shared(p(idx), p(cn), p(idx), p(cn), K, k, p(sh))
torch.cuda.synchronize()
assert bool((sh == cn).all())
form = "plain" if os.environ.get("FASTF_COEXPR_MFMA", "1")[:1] == "0" else "mfma"
tiles = (K_pad // 32) * (K_pad // 32 + 1) // 2
ops = 2.0 * 32 * 32 * tiles * ((n + 31) // 32 * 32) * P * P
print("%s, chunk %d: %d cells x %d genes, %d plane(s), k %d: fastf_dev_coexpr_sums min %.4f s median %.4f s (%.2f T integer op/s at the minimum), "
      "fastf_dev_coexpr_select min %.4f s median %.4f s" % (form, chunk, n, K, P, k, t_sums[0], t_sums[1], ops / t_sums[0] / 1e12, t_sel[0], t_sel[1]))
if a.host:
    rows = [hostmem.to_host(t).astype(np.uint32) for t in (feat, cell, cnt)]
    t = time.time()
    h_idx, h_cnt, h_D, h_S = sweep.coexpression_from_coo(rows, n, sweep.neighbors_slot_map(np.arange(K), K), K, k)
    th = time.time() - t
    same = (bool((hostmem.to_host(D).view(np.uint64).reshape(K, K) == h_D).all()) and bool((hostmem.to_host(S).view(np.uint64) == h_S).all())
            and bool((hostmem.to_host(idx).view(np.uint32).reshape(K, k) == h_idx).all()) and bool((hostmem.to_host(cn).view(np.uint32) == h_cnt).all()))
    print("host twin fastf_coexpr_from_coo on the same rows: %.3f s (one thread); device sums + select at the minimum: %.4f s, %.0f times faster; same D, S and sets: %s"
          % (th, t_sums[0] + t_sel[0], th / (t_sums[0] + t_sel[0]), same))
    assert same
e.close()
