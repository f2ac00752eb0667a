"""The two device calls of --pseudotime beside the call of --neighbors they sit behind, on one large matrix: --cells cells x 2000 genes,
5 % of the entries non-zero, counts below 2^7 (one plane).  fastf_dev_neighbors lays down the neighbour sets (k = 15); t is a random
permutation of the doubled ranks with a tenth of the cells left without a value.  After a first call of each, fastf_dev_neighbors,
fastf_dev_ptime_medians and fastf_dev_ptime_census are timed by the wall clock with a synchronise behind the call, interleaved, five
times each; the medians are printed, and the census is checked against n (n - 1) / 2 pairs.

    python tools/ptime_kernels.py --cells 25000
    python tools/ptime_kernels.py --cells 50000
(profiles/ptime_notes/: the printed lines)"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import fastf_amd as F
from fastf_amd import sweep
ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=25_000)
ap.add_argument("--genes", type=int, default=2000)
ap.add_argument("--k", type=int, default=15)
a = ap.parse_args()
n, K, k = a.cells, a.genes, a.k
e = F.Engine(np.arange(1, 101, dtype=np.uint64) | (np.uint64(1) << np.uint64(62)), np.arange(1, 51, dtype=np.uint64) | (np.uint64(2) << np.uint64(62)), umi_max_bases=12)
g = torch.Generator(device="cuda"); g.manual_seed(1)
per = K // 20                                              # 5 % of the genes per cell, one in every stride of 20
cell = torch.arange(1, n + 1, device="cuda", dtype=torch.int32).repeat_interleave(per)
feat = (torch.arange(per, device="cuda", dtype=torch.int32) * 20).repeat(n) + torch.randint(1, 21, (n * per,), device="cuda", dtype=torch.int32, generator=g)
cnt = torch.randint(2, 100, (n * per,), device="cuda", dtype=torch.int32, generator=g)
d_n = torch.tensor([n * per], dtype=torch.int64, device="cuda")
sm = torch.from_numpy(sweep.neighbors_slot_map(np.arange(K), K).view(np.int16)).cuda()
p = lambda t: t.data_ptr()
n_pad, K_pad = sweep.neighbors_pad(n, K)
P = e.dev_neighbor_planes(p(feat), p(cell), p(cnt), p(d_n), p(sm), K, n, K)
assert P == 1
planes = torch.empty(P * n_pad * K_pad, dtype=torch.uint8, device="cuda")
e.dev_neighbor_planes(p(feat), p(cell), p(cnt), p(d_n), p(sm), K, n, K, p(planes), planes.numel())
idx = torch.zeros(n * k, dtype=torch.int32, device="cuda")
cn, est, valued = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
norms = torch.zeros(n, dtype=torch.int64, device="cuda")
out = torch.zeros(8, dtype=torch.int64, device="cuda")
rank = (torch.randperm(n, device="cuda", generator=g).to(torch.int32) + 1) * 2
rank[torch.rand(n, device="cuda", generator=g) < 0.1] = 0


def neighbors():
    e.dev_neighbors(p(planes), P, n, K, k, p(idx), p(cn), p(norms))


def medians():
    e.dev_ptime_medians(p(idx), p(cn), p(rank), n, k, p(est), p(valued))


def census():
    e.dev_ptime_census(p(est), p(rank), n, p(out))


def timed(fn):
    torch.cuda.synchronize()
    t = time.time()
    fn()
    torch.cuda.synchronize()
    return time.time() - t


neighbors(); medians(); census()                            # a first call of each
tn, tm, tc = [], [], []
for _ in range(5):
    tn.append(timed(neighbors)); tm.append(timed(medians)); tc.append(timed(census))
c = [int(x) for x in out.cpu()[:7]]
cells = int(((est != 0) & (rank != 0)).sum())
assert c[5] == cells and sum(c[:5]) == cells * (cells - 1) // 2
print("%d cells x %d genes, 1 plane, k %d: fastf_dev_neighbors %.4f s, fastf_dev_ptime_medians %.6f s, fastf_dev_ptime_census %.6f s (medians of 5); "
      "%d cells in the census, %d pairs in %d workgroups, conc %d disc %d" %
      (n, K, k, float(np.median(tn)), float(np.median(tm)), float(np.median(tc)), cells, cells * (cells - 1) // 2,
       (lambda T: T * (T + 1) // 2)((n + sweep.PTIME_TILE - 1) // sweep.PTIME_TILE), c[0], c[1]))
e.close()
