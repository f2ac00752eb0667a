"""replicate seeds in one process against one process per seed: seconds from process start to exit on the generated BAM and the grid
of tools/sweep_bench.py, --runs interleaved runs each, medians:

    baseline    `fastF sweep -s <seed>` once per seed with --baseline-fastf (the binary of the commit to compare against), summed
    replicates  `fastF sweep --reps <n>` of this tree, one process, with its FASTF_PROFILE stage lines; once more with
                FASTF_RES_NO_REUSE=1 (fresh buffers and a fresh blocked copy for every (cell rate, seed) pair)
    single      `fastF sweep -s 926` without the new options, baseline binary against this tree's

each in the full form and with --summary-only.

    python tools/reps_bench.py --records 20000000 --baseline-fastf <parent>/fastf_amd/bin/fastF --out profiles/reps_notes
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=926)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--forms", default="summary,full")
    ap.add_argument("--dir", default="/dev/shm/reps_bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reps_notes"))
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
    io = ["-b", bam, "-a", bar, "-f", feat, "-c", a.cells, "-r", a.depths]
    seeds = [a.seed + k for k in range(a.reps)]
    lines = ["%d records, BAM %.2f GB, grid %s x %s, seeds %s, %d interleaved runs each; baseline binary %s" %
             (a.records, os.path.getsize(bam) / 1e9, a.cells, a.depths, ",".join(str(s) for s in seeds), a.runs, base)]
    rc = 0
    med = statistics.median
    fmt = lambda v: " ".join("%.3f" % t for t in v)  # noqa: E731
    try:
        for form in a.forms.split(","):
            extra = ["--summary-only"] if form == "summary" else []
            t_base, t_reps, t_fresh, t_one_base, t_one = [], [], [], [], []
            prof, prof_fresh = "", ""
            for _ in range(a.runs):
                tot, tables = 0.0, {}
                for s in seeds:
                    od = os.path.join(a.dir, "base")
                    dt, p = run([base, "sweep"] + io + ["-o", od, "-s", str(s)] + extra)
                    if p.returncode:
                        print(p.stderr)
                        return 1
                    tot += dt
                    tables[s] = open(os.path.join(od, "sweep.tsv")).read().split("\n")[1:-1]
                    shutil.rmtree(od)
                t_base.append(tot)
                for which in ("fresh", "reps"):
                    od = os.path.join(a.dir, which)
                    env = {"FASTF_PROFILE": "1"}
                    if which == "fresh":
                        env["FASTF_RES_NO_REUSE"] = "1"
                    dt, p = run([fastf, "sweep"] + io + ["-o", od, "--reps", str(a.reps), "-s", str(a.seed)] + extra, env)
                    if p.returncode:
                        print(p.stderr)
                        return 1
                    # the rows of the replicate run are the rows of the per-seed runs
                    rows = open(os.path.join(od, "sweep.tsv")).read().split("\n")[1:-1]
                    for s in seeds:
                        if [r for r in rows if r.split("\t")[2] == str(s)] != tables[s]:
                            print("the rows of seed %d differ from the baseline's" % s)
                            return 1
                    text = "".join(ln + "\n" for ln in p.stderr.split("\n") if ln.startswith("[sweep]"))
                    if which == "fresh":
                        t_fresh.append(dt); prof_fresh = text
                    else:
                        t_reps.append(dt); prof = text
                    shutil.rmtree(od)
                for binary, acc in ((base, t_one_base), (fastf, t_one)):
                    od = os.path.join(a.dir, "one")
                    dt, p = run([binary, "sweep"] + io + ["-o", od, "-s", str(a.seed)] + extra)
                    if p.returncode:
                        print(p.stderr)
                        return 1
                    acc.append(dt)
                    shutil.rmtree(od)
            lines += ["", "== %s ==" % ("sweep --summary-only" if extra else "sweep with matrices"),
                      "baseline, %d processes summed: runs %s, median %.3f s (spread %.3f s)" % (a.reps, fmt(t_base), med(t_base), max(t_base) - min(t_base)),
                      "--reps %d, one process: runs %s, median %.3f s (spread %.3f s; %.2f x the baseline's speed)" %
                      (a.reps, fmt(t_reps), med(t_reps), max(t_reps) - min(t_reps), med(t_base) / med(t_reps)),
                      prof.rstrip("\n"),
                      "--reps %d with FASTF_RES_NO_REUSE=1: runs %s, median %.3f s" % (a.reps, fmt(t_fresh), med(t_fresh)),
                      prof_fresh.rstrip("\n"),
                      "single seed, baseline binary: runs %s, median %.3f s (spread %.3f s)" % (fmt(t_one_base), med(t_one_base), max(t_one_base) - min(t_one_base)),
                      "single seed, this tree: runs %s, median %.3f s (spread %.3f s)" % (fmt(t_one), med(t_one), max(t_one) - min(t_one))]
            # the condition: faster than the sum; it holds beyond the spread only when the slowest replicate run beats the fastest sum
            if med(t_reps) >= med(t_base):
                lines.append("THE REPLICATE RUN IS NOT FASTER THAN THE SUMMED BASELINE")
                rc = 1
            elif max(t_reps) >= min(t_base):
                lines.append("faster by the medians, but the runs overlap: slowest replicate run %.3f s, fastest summed baseline %.3f s" % (max(t_reps), min(t_base)))
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    open(os.path.join(a.out, "reps_vs_per_seed_%dM.txt" % (a.records // 1_000_000)), "w").write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
