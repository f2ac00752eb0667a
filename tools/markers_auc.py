"""Wall time of one fastf_dev_marker_auc call on random byte planes: --cells cells x --genes genes of A, --nonzero the share of non-zero
counts, --labels labels, --planes 1 or 2, in the form FASTF_MARKERS_LDS selects (unset: the accumulators in LDS where they fit; 0:
global atomics alone).  The result is checked against the host twin.  (profiles/markers_notes/: the printed lines)"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import fastf_amd as F
from fastf_amd import sweep
ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=50_000)
ap.add_argument("--genes", type=int, default=2000)
ap.add_argument("--labels", type=int, default=30)
ap.add_argument("--planes", type=int, default=1)
ap.add_argument("--nonzero", type=float, default=0.05)
a = ap.parse_args()
n, K, L, P = a.cells, a.genes, a.labels, a.planes
rng = np.random.default_rng(1)
counts = rng.geometric(0.3, size=(n, K)).astype(np.int64)                     # small counts, as UMIs are
if P == 2:
    wide = rng.random((n, K)) < 0.02
    counts[wide] = rng.integers(128, 16384, size=int(wide.sum()))
counts = np.minimum(counts, 128 ** P - 1)
counts[rng.random((n, K)) >= a.nonzero] = 0
lab = rng.integers(0, L + 1, size=n).astype(np.uint8)
planes = sweep.marker_planes(counts, P)
e = F.Engine(np.arange(1, 101, dtype=np.uint64) | (np.uint64(1) << np.uint64(62)), np.arange(1, 51, dtype=np.uint64) | (np.uint64(2) << np.uint64(62)), umi_max_bases=12)
d_planes, d_lab = torch.from_numpy(planes.reshape(-1)).cuda(), torch.from_numpy(lab).cuda()
W = L * K
out = [torch.zeros(W, dtype=torch.int64, device="cuda"), torch.zeros(W, dtype=torch.int32, device="cuda"), torch.zeros(W, dtype=torch.int64, device="cuda"),
       torch.zeros(L, dtype=torch.int32, device="cuda")]
p = lambda t: t.data_ptr()
times = []
for _ in range(6):
    torch.cuda.synchronize()
    t = time.time()
    e.dev_marker_auc(p(d_planes), P, n, K, p(d_lab), L, p(out[0]), p(out[1]), p(out[2]), p(out[3]))
    torch.cuda.synchronize()
    times.append(time.time() - t)
want = sweep.marker_auc(planes, P, n, K, lab, L)
got = [o.cpu().numpy().view(u) for o, u in zip(out, (np.uint64, np.uint32, np.uint64, np.uint32))]
assert all((g.reshape(w.shape) == w).all() for g, w in zip(got, want))
form = "LDS" if sweep.marker_auc_form(P, L) == 1 else "global atomics"
n_pad, K_pad = sweep.neighbors_pad(n, K)
floor = 2 * P * n_pad * K_pad / 6.3e12
med = sorted(times[1:])[2]
print("%s, %d plane(s): %d cells x %d genes, %.0f %% non-zero, %d labels: fastf_dev_marker_auc first call %.6f s, then min %.6f s median %.6f s of 5; "
      "traffic floor (2 passes over %d x %d x %d bytes at 6.3 TB/s) %.6f s, median / floor %.1f" %
      (form, P, n, K, 100 * a.nonzero, L, times[0], min(times[1:]), med, P, n_pad, K_pad, floor, med / floor))
e.close()
