"""cap against sweep: seconds from process start to exit on the generated 20 M-record BAM of tools/sweep_bench.py (50 000 barcodes x
36 601 genes), the same cell rates, as many caps as depth rates, --runs runs each, with matrices and with --summary-only, and the
FASTF_PROFILE stage lines of the last run of each.  --baseline-fastf: the fastF whose `sweep` is the yardstick (the parent commit's).

    python tools/cap_bench.py --records 20000000 --baseline-fastf <parent>/fastf_amd/bin/fastF --out profiles/cap_notes
"""
import argparse
import os
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastf_amd import synth  # noqa: E402
from sweep_bench import run  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--cells", default="0.25,0.5,0.75,1")
    ap.add_argument("--depths", default="0.1,0.25,0.5,0.75,1")
    ap.add_argument("--caps", default="30,100,300,1000,1000000")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm/cap_bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cap_notes"))
    ap.add_argument("--baseline-fastf", default=None)
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
    io = ["-b", bam, "-a", bar, "-f", feat]
    jobs = [("sweep with matrices (%s)" % base, [base, "sweep"] + io + ["-c", a.cells, "-r", a.depths], "sweep.tsv"),
            ("sweep --summary-only", [base, "sweep"] + io + ["-c", a.cells, "-r", a.depths, "--summary-only"], "sweep.tsv"),
            ("cap with matrices (%s)" % fastf, [fastf, "cap"] + io + ["-c", a.cells, "-n", a.caps], "cap.tsv"),
            ("cap --summary-only", [fastf, "cap"] + io + ["-c", a.cells, "-n", a.caps, "--summary-only"], "cap.tsv")]
    lines = ["%d records, BAM %.2f GB, cell rates %s, depth rates %s / caps %s, %d runs each, interleaved" %
             (a.records, os.path.getsize(bam) / 1e9, a.cells, a.depths, a.caps, a.runs)]
    times = {j[0]: [] for j in jobs}
    prof, tables, sizes = {}, {}, {}
    try:
        for _ in range(a.runs):
            for name, cmd, table in jobs:
                od = os.path.join(a.dir, "out")
                dt, p = run(cmd + ["-o", od], {"FASTF_PROFILE": "1"})
                if p.returncode:
                    print(name, p.stderr)
                    return 1
                times[name].append(dt)
                prof[name] = "".join(ln + "\n" for ln in p.stderr.split("\n") if ln.startswith("[")).rstrip("\n")
                tables[name] = open(os.path.join(od, table)).read()
                sizes[name] = sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(od) for f in fs)
                shutil.rmtree(od)
        for name, _, _ in jobs:
            t = times[name]
            lines += ["%s: runs %s, median %.3f s, spread %.3f s, %.1f MB written" %
                      (name, " ".join("%.3f" % x for x in t), statistics.median(t), max(t) - min(t), sizes[name] / 1e6), prof[name]]
        lines += ["cap.tsv:", tables[jobs[2][0]].rstrip("\n"), "sweep.tsv:", tables[jobs[0][0]].rstrip("\n")]
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    open(os.path.join(a.out, "cap_vs_sweep_%dM.txt" % (a.records // 1_000_000)), "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
