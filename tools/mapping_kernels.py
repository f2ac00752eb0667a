"""The device call of --mapping beside the call of --neighbors it is modelled on, on one large matrix: --cells cells x 2000 genes, 5 % of
the entries non-zero, counts below 2^7 (one plane) or below 2^14 (two planes, --planes 2).  The full rows' planes are laid down once; the
point is a thinned copy (every count halved, rounded up: the same planes).  After a first call of each, fastf_dev_mapping (the two
maxima, one read-back, the diagonal and the Gram kernel) and fastf_dev_neighbors (the norms, one read-back, the Gram kernel) on the
SAME full planes are timed by the wall clock, interleaved, five times each; the medians and their ratio are printed.  Both do
2 * cells^2 * K_pad * planes^2 multiply-adds; the mapping adds one 128-bit compare per live candidate.

    python tools/mapping_kernels.py --cells 25000 --planes 1
    FASTF_MAPPING_MFMA=0 FASTF_NEIGHBORS_MFMA=0 python tools/mapping_kernels.py --cells 25000 --planes 1
(profiles/mapping_notes/: the printed lines)"""
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
cnt = torch.randint(2 if a.planes == 1 else 300, 100 if a.planes == 1 else 16000, (n * per,), device="cuda", dtype=torch.int32, generator=g)
d_n = torch.tensor([n * per], dtype=torch.int64, device="cuda")
sm = torch.from_numpy(sweep.neighbors_slot_map(np.arange(K), K).view(np.int16)).cuda()
p = lambda t: t.data_ptr()
n_pad, K_pad = sweep.neighbors_pad(n, K)
planes = []
for c in (cnt, (cnt + 1) // 2):                             # the full rows, the point
    P = e.dev_neighbor_planes(p(feat), p(cell), p(c), p(d_n), p(sm), K, n, K)
    assert P == a.planes
    planes.append(torch.empty(P * n_pad * K_pad, dtype=torch.uint8, device="cuda"))
    e.dev_neighbor_planes(p(feat), p(cell), p(c), p(d_n), p(sm), K, n, K, p(planes[-1]), planes[-1].numel())
P = a.planes
idx, midx = (torch.zeros(n * k, dtype=torch.int32, device="cuda") for _ in range(2))
cn, mcn, rank, hood = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(4))
norms, sd = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))


def neighbors():
    e.dev_neighbors(p(planes[0]), P, n, K, k, p(idx), p(cn), p(norms))


def mapping():
    e.dev_mapping(p(planes[1]), P, p(planes[0]), P, n, K, k, p(norms), p(midx), p(mcn), p(sd), p(rank))


def timed(fn):
    torch.cuda.synchronize()
    t = time.time()
    fn()
    torch.cuda.synchronize()
    return time.time() - t


neighbors(); mapping()                                      # a first call of each
tn, tm = [], []
for _ in range(5):
    tn.append(timed(neighbors)); tm.append(timed(mapping))
e.dev_neighbors_shared(p(midx), p(mcn), p(idx), p(cn), n, k, p(hood))
torch.cuda.synchronize()
assert int(mcn.min()) == k and int(rank.max()) < n
mn, mm = float(np.median(tn)), float(np.median(tm))
form = "plain" if os.environ.get("FASTF_MAPPING_MFMA", "1")[:1] == "0" else "mfma"
print("%s: %d cells x %d genes, %d plane(s), k %d: fastf_dev_neighbors %.4f s, fastf_dev_mapping %.4f s (medians of 5), ratio %.3f; self_top1 %.4f, mean hood %.2f" %
      (form, n, K, P, k, mn, mm, mm / mn, float((rank == 0).float().mean()), float(hood.float().mean())))
e.close()
