"""level against cap: seconds from process start to exit on the generated BAM of tools/sweep_bench.py (50 000 barcodes x 36 601
genes), a 4 x 5 grid, --runs interleaved runs each, with matrices and with --summary-only, the FASTF_PROFILE stage lines of the last
run of each, and from level's per-point lines the probing passes per point, the seconds of search per point and the ratio of a
probing pass to the point's own pass.  --baseline-fastf: the fastF whose `cap` is the yardstick (the parent commit's).

    python tools/level_bench.py --records 20000000 --baseline-fastf <parent>/fastf_amd/bin/fastF --out profiles/level_notes
"""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastf_amd import synth  # noqa: E402
from sweep_bench import run  # noqa: E402


def search_numbers(stderr):
    """(points, probing passes, seconds of search, seconds of the points' own passes) from the `[level] point` lines"""
    pts = re.findall(r"\[level\] point \S+: (\d+) probing passes, search ([0-9.]+) s, the point's own pass ([0-9.]+) s", stderr)
    return len(pts), sum(int(p[0]) for p in pts), sum(float(p[1]) for p in pts), sum(float(p[2]) for p in pts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--cells", default="0.25,0.5,0.75,1")
    ap.add_argument("--caps", default="30,100,300,1000,1000000")
    ap.add_argument("--umis", default="20,60,150,400,1000000")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm/level_bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_notes"))
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
    jobs = [("cap with matrices (%s)" % base, [base, "cap"] + io + ["-c", a.cells, "-n", a.caps], "cap.tsv"),
            ("cap --summary-only (%s)" % base, [base, "cap"] + io + ["-c", a.cells, "-n", a.caps, "--summary-only"], "cap.tsv"),
            ("level with matrices (%s)" % fastf, [fastf, "level"] + io + ["-c", a.cells, "-m", a.umis], "level.tsv"),
            ("level --summary-only", [fastf, "level"] + io + ["-c", a.cells, "-m", a.umis, "--summary-only"], "level.tsv")]
    if base != fastf:                                       # this build's own cap next to the yardstick's: the split of fastf_res_point_run must not move it
        jobs += [("cap with matrices (%s)" % fastf, [fastf, "cap"] + io + ["-c", a.cells, "-n", a.caps], "cap.tsv"),
                 ("cap --summary-only (%s)" % fastf, [fastf, "cap"] + io + ["-c", a.cells, "-n", a.caps, "--summary-only"], "cap.tsv")]
    lines = ["%d records, BAM %.2f GB, cell rates %s, caps %s / UMI caps %s, %d runs each, interleaved" %
             (a.records, os.path.getsize(bam) / 1e9, a.cells, a.caps, a.umis, a.runs)]
    times = {j[0]: [] for j in jobs}
    prof, tables, sizes, search = {}, {}, {}, {}
    try:
        for _ in range(a.runs):
            for name, cmd, table in jobs:
                od = os.path.join(a.dir, "out")
                dt, p = run(cmd + ["-o", od], {"FASTF_PROFILE": "1"})
                if p.returncode:
                    print(name, p.stderr)
                    return 1
                times[name].append(dt)
                prof[name] = "".join(ln + "\n" for ln in p.stderr.split("\n") if ln.startswith("[") and "] point " not in ln).rstrip("\n")
                search[name] = search_numbers(p.stderr)
                tables[name] = open(os.path.join(od, table)).read()
                sizes[name] = sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(od) for f in fs)
                shutil.rmtree(od)
        for name, _, _ in jobs:
            t = times[name]
            lines += ["%s: runs %s, median %.3f s, spread %.3f s, %.1f MB written" %
                      (name, " ".join("%.3f" % x for x in t), statistics.median(t), max(t) - min(t), sizes[name] / 1e6), prof[name]]
            n, passes, s_search, s_own = search[name]
            if n and passes:
                lines += ["  search: %d points, %.1f probing passes a point, %.4f s of search a point, a probing pass %.5f s against the point's own "
                          "pass %.5f s (ratio %.2f)" % (n, passes / n, s_search / n, s_search / passes, s_own / n, (s_search / passes) / (s_own / n))]
        lines += ["level.tsv:", tables[jobs[2][0]].rstrip("\n"), "cap.tsv:", tables[jobs[0][0]].rstrip("\n")]
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    open(os.path.join(a.out, "level_vs_cap_%dM.txt" % (a.records // 1_000_000)), "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
