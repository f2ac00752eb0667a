"""sweep against bam2db point by point: seconds from process start to exit on a generated Cell-Ranger-shaped BAM (tools/gen_bam.c,
50 000 barcodes x 36 601 genes, 12-base UMIs, 91-base reads), a grid of cell x depth rates, median of --runs runs:

    baseline   `fastF bam2db` once per point, times summed (--baseline-fastf: the binary of the commit to compare against)
    sweep      `fastF sweep` with matrices, and `fastF sweep --summary-only`, with their FASTF_PROFILE stage lines

    python tools/sweep_bench.py --records 20000000 --out profiles/sweep_notes
"""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastf_amd import synth  # noqa: E402


def run(cmd, env=None, timeout=900):
    e = dict(os.environ)
    e.update(env or {})
    t = time.time()
    p = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=timeout)
    return time.time() - t, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--cells", default="0.25,0.5,0.75,1")
    ap.add_argument("--depths", default="0.1,0.25,0.5,0.75,1")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm/sweep_bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_notes"))
    ap.add_argument("--baseline-fastf", default=None, help="fastF of the commit to compare against (default: this tree's)")
    ap.add_argument("--gen-bam", default=os.path.join(ROOT, "build", "gen_bam"))
    a = ap.parse_args()
    fastf = os.path.join(ROOT, "fastf_amd", "bin", "fastF")
    base = a.baseline_fastf or fastf
    os.makedirs(a.dir, exist_ok=True)
    os.makedirs(a.out, exist_ok=True)
    bar, feat, bam = (os.path.join(a.dir, n) for n in ("bar.tsv", "feat.tsv", "in.bam"))
    bt, ft, _, _ = synth.make_lists(50_000, 36_601, seed=77)
    open(bar, "wb").write(bt)
    open(feat, "wb").write(ft)
    if not os.path.exists(a.gen_bam):
        subprocess.check_call(["gcc", "-O2", "-o", a.gen_bam, os.path.join(ROOT, "tools", "gen_bam.c"), "-lz", "-lpthread"])
    subprocess.check_call([a.gen_bam, bam, bar, feat, str(a.records), "7", "12", "91", "16"], stdout=subprocess.DEVNULL)
    cells, depths = a.cells.split(","), a.depths.split(",")
    io = ["-b", bam, "-a", bar, "-f", feat]
    lines = ["%d records, BAM %.2f GB, grid %s x %s, %d runs each" % (a.records, os.path.getsize(bam) / 1e9, a.cells, a.depths, a.runs)]
    rc = 0
    try:
        t_base, t_full, t_sum, prof_full, prof_sum = [], [], [], "", ""
        for _ in range(a.runs):
            tot = 0.0
            for c in cells:
                for r in depths:
                    od = os.path.join(a.dir, "base")
                    os.makedirs(od, exist_ok=True)
                    dt, p = run([base, "bam2db"] + io + ["-o", od, "-c", c, "-r", r])
                    if p.returncode:
                        print(p.stderr)
                        return 1
                    tot += dt
                    shutil.rmtree(od)
            t_base.append(tot)
            od = os.path.join(a.dir, "full")
            dt, p = run([fastf, "sweep"] + io + ["-o", od, "-c", a.cells, "-r", a.depths], {"FASTF_PROFILE": "1"})
            if p.returncode:
                print(p.stderr)
                return 1
            t_full.append(dt)
            prof_full = "".join(ln + "\n" for ln in p.stderr.split("\n") if ln.startswith("[sweep]"))
            table = open(os.path.join(od, "sweep.tsv")).read()
            shutil.rmtree(od)
            od = os.path.join(a.dir, "summary")
            dt, p = run([fastf, "sweep"] + io + ["-o", od, "-c", a.cells, "-r", a.depths, "--summary-only"], {"FASTF_PROFILE": "1"})
            if p.returncode or open(os.path.join(od, "sweep.tsv")).read() != table:
                print("summary-only run failed or its table differs\n" + p.stderr)
                return 1
            t_sum.append(dt)
            prof_sum = "".join(ln + "\n" for ln in p.stderr.split("\n") if ln.startswith("[sweep]"))
            shutil.rmtree(od)
        n_pts = len(cells) * len(depths)
        lines += ["bam2db once per point (%s), %d points summed: runs %s, median %.3f s (%.3f s a point)" %
                  (base, n_pts, " ".join("%.3f" % t for t in t_base), statistics.median(t_base), statistics.median(t_base) / n_pts),
                  "sweep with matrices: runs %s, median %.3f s" % (" ".join("%.3f" % t for t in t_full), statistics.median(t_full)),
                  prof_full.rstrip("\n"),
                  "sweep --summary-only: runs %s, median %.3f s" % (" ".join("%.3f" % t for t in t_sum), statistics.median(t_sum)),
                  prof_sum.rstrip("\n"), "sweep.tsv:", table.rstrip("\n")]
        if statistics.median(t_full) > statistics.median(t_base):
            lines.append("FULL SWEEP SLOWER THAN THE SUMMED BASELINE")
            rc = 1
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    open(os.path.join(a.out, "sweep_vs_bam2db_%dM.txt" % (a.records // 1_000_000)), "w").write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
