"""The device calls of --gene-fidelity on one large point, for a kernel trace: 40 M rows of 50 000 cells (800 rows a cell, 36 601
features, point == full), five rounds of fastf_dev_fidelity (the yardstick of the walk), fastf_dev_partner_counts,
fastf_dev_gene_summary (the yardstick of the accumulation) and fastf_dev_gene_moments on the same rows; the results are checked.

    rocprofv3 --kernel-trace --stats --output-format csv -d out -o gf -- python tools/gene_fidelity_kernels.py

(profiles/gene_fidelity_notes/kernels_40M.txt: the rows of out/gf_kernel_stats.csv and the launches of out/gf_kernel_trace.csv)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import fastf_amd as F
n_cells, per, nf = 50_000, 800, 36_601
cells = np.arange(1, n_cells + 1, dtype=np.uint64) | (np.uint64(1) << np.uint64(62))
feats = np.arange(1, nf + 1, dtype=np.uint64) | (np.uint64(2) << np.uint64(62))
e = F.Engine(cells, feats, umi_max_bases=12)
g = torch.Generator(device="cuda"); g.manual_seed(1)
n = n_cells * per
cell = torch.arange(1, n_cells + 1, device="cuda", dtype=torch.int32).repeat_interleave(per)
feat = (torch.arange(per, device="cuda", dtype=torch.int32) * 45).repeat(n_cells) + torch.randint(1, 46, (n,), device="cuda", dtype=torch.int32, generator=g)
cnt = torch.randint(1, 50, (n,), device="cuda", dtype=torch.int32, generator=g)
d_n = torch.tensor([n], dtype=torch.int64, device="cuda")
x = torch.zeros(n, dtype=torch.int32, device="cuda")
sxy, syy = torch.zeros(n_cells, dtype=torch.int64, device="cuda"), torch.zeros(n_cells, dtype=torch.int64, device="cuda")
cpg, upg = torch.zeros(nf, dtype=torch.int32, device="cuda"), torch.zeros(nf, dtype=torch.int64, device="cuda")
gab, gbb = torch.zeros(nf, dtype=torch.int64, device="cuda"), torch.zeros(nf, dtype=torch.int64, device="cuda")
p = lambda t: t.data_ptr()
for r in range(5):
    e.dev_fidelity(p(feat), p(cell), p(cnt), p(d_n), p(feat), p(cell), p(cnt), p(d_n), n_cells, p(sxy), p(syy))
    e.dev_partner_counts(p(feat), p(cell), p(cnt), p(d_n), p(feat), p(cell), p(d_n), p(x))
    e.dev_gene_summary(p(feat), p(cnt), p(d_n), nf, p(cpg), p(upg))
    e.dev_gene_moments(p(feat), p(x), p(cnt), p(d_n), nf, p(gab), p(gbb))
    torch.cuda.synchronize()
assert bool((x == cnt).all()) and int(gab.sum()) == int((cnt.long() * cnt.long()).sum()) == int(gbb.sum()) and int(upg.sum()) == int(cnt.long().sum())
print("ok: %d rows" % n)
e.close()
