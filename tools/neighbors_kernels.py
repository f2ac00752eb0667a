"""The device calls of --neighbors on one large matrix, for a kernel trace: --cells cells x 2000 genes, 5 % of the entries non-zero,
counts below 2^7 (one plane) or below 2^14 (two planes, --planes 2); fastf_dev_neighbor_planes once, then fastf_dev_neighbors in the
form FASTF_NEIGHBORS_MFMA selects and fastf_dev_neighbors_shared of the set with itself, which must give k everywhere.

    rocprofv3 --kernel-trace --stats --output-format csv -d out -o nb -- python tools/neighbors_kernels.py --cells 25000 --planes 1
    FASTF_NEIGHBORS_MFMA=0 rocprofv3 ... -- python tools/neighbors_kernels.py --cells 25000 --planes 1

Without a profiler the wall time of fastf_dev_neighbors (the norms, one read-back and the Gram kernel) is printed, and from it the
integer rate of the dot products: 2 * cells^2 * K_pad * planes^2 operations.
(profiles/neighbors_notes/: the rows of out/nb_kernel_stats.csv)"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import fastf_amd as F
from fastf_amd import sweep
ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=25_000)
ap.add_argument("--genes", type=int, default=2000)
ap.add_argument("--planes", type=int, default=1)
ap.add_argument("--k", type=int, default=15)
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
n_pad, K_pad = sweep.neighbors_pad(n, K)
P = e.dev_neighbor_planes(p(feat), p(cell), p(cnt), p(d_n), p(sm), K, n, K)
assert P == a.planes
planes = torch.empty(P * n_pad * K_pad, dtype=torch.uint8, device="cuda")
e.dev_neighbor_planes(p(feat), p(cell), p(cnt), p(d_n), p(sm), K, n, K, p(planes), planes.numel())
idx = torch.zeros(n * k, dtype=torch.int32, device="cuda")
cn, sh = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
norms = torch.zeros(n, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
t = time.time()
e.dev_neighbors(p(planes), P, n, K, k, p(idx), p(cn), p(norms))
torch.cuda.synchronize()
dt = time.time() - t
e.dev_neighbors_shared(p(idx), p(cn), p(idx), p(cn), n, k, p(sh))
torch.cuda.synchronize()
assert bool((sh == cn).all()) and int(cn.min()) == k
form = "plain" if os.environ.get("FASTF_NEIGHBORS_MFMA", "1")[:1] == "0" else "mfma"
print("%s: %d cells x %d genes, %d plane(s), k %d: fastf_dev_neighbors %.3f s, %.1f T integer op/s" % (form, n, K, P, k, dt, 2.0 * n * n * K_pad * P * P / dt / 1e12))
e.close()
