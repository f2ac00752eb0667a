"""Wall time of one fastf_dev_label_votes call on random neighbour sets: --cells cells, k slots each, --labels labels, in the form
FASTF_LABELS_LDS selects (unset: the confusion counts through LDS; 0: global atomics alone).  The result is checked against the host
twin.  (profiles/labels_notes/: the printed lines)"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import fastf_amd as F
from fastf_amd import sweep
ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=50_000)
ap.add_argument("--k", type=int, default=15)
ap.add_argument("--labels", type=int, default=30)
a = ap.parse_args()
n, k, L = a.cells, a.k, a.labels
rng = np.random.default_rng(1)
idx = np.sort((np.arange(n)[:, None] + 1 + rng.choice(n - 1, size=(n, k))) % n, axis=1).astype(np.uint32)     # never the cell itself
cnt = rng.integers(0, k + 1, size=n).astype(np.uint32)
idx[np.arange(k)[None, :] >= cnt[:, None]] = 0xFFFFFFFF
lab = rng.integers(0, L + 1, size=n).astype(np.uint8)
e = F.Engine(np.arange(1, 101, dtype=np.uint64) | (np.uint64(1) << np.uint64(62)), np.arange(1, 51, dtype=np.uint64) | (np.uint64(2) << np.uint64(62)), umi_max_bases=12)
d = [torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda() for x in (idx.reshape(-1), cnt, lab)]
out = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(3)]
conf = torch.zeros(L * (L + 1), dtype=torch.int32, device="cuda")
p = lambda t: t.data_ptr()
times = []
for _ in range(5):
    torch.cuda.synchronize()
    t = time.time()
    e.dev_label_votes(p(d[0]), p(d[1]), p(d[2]), n, k, L, p(out[0]), p(out[1]), p(out[2]), p(conf))
    torch.cuda.synchronize()
    times.append(time.time() - t)
want = sweep.label_votes(idx, cnt, lab, k, L)
assert all((o.cpu().numpy() == w).all() for o, w in zip(out, want[:3])) and (conf.cpu().numpy().view(np.uint32).reshape(L, L + 1) == want[3]).all()
form = "global atomics" if os.environ.get("FASTF_LABELS_LDS", "1")[:1] == "0" else "LDS"
print("%s: %d cells, k %d, %d labels: fastf_dev_label_votes first call %.6f s, then min %.6f s median %.6f s of 4" % (form, n, k, L, times[0], min(times[1:]), sorted(times[1:])[2]))
e.close()
