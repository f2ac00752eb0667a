"""--neighbors end to end: `fastF sweep` on the generated BAM and the grid of tools/sweep_bench.py, seconds from process start to
exit, --runs interleaved rounds of: the baseline binary and this tree's without the flag (summary-only and with matrices), then this
tree's with --neighbors both ways, with the FASTF_PROFILE=1 stage lines of the last round.

    python tools/neighbors_bench.py --baseline-fastf <fastF of the parent commit> --out profiles/neighbors_notes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--cells", default="0.25,0.5,0.75,1")
    ap.add_argument("--depths", default="0.1,0.25,0.5,0.75,1")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm/neighbors_bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbors_notes"))
    ap.add_argument("--baseline-fastf", default=None, help="fastF of the commit to compare against (default: this tree's)")
    ap.add_argument("--gen-bam", default=os.path.join(ROOT, "build", "gen_bam"))
    a = ap.parse_args()
    fastf = os.path.join(ROOT, "fastf_amd", "bin", "fastF")
    base = a.baseline_fastf or fastf
    os.makedirs(a.dir, exist_ok=True)
    os.makedirs(a.out, exist_ok=True)
    bar, feat, bam, od = (os.path.join(a.dir, n) for n in ("bar.tsv", "feat.tsv", "in.bam", "out"))
    bt, ft, _, _ = synth.make_lists(50_000, 36_601, seed=77)
    open(bar, "wb").write(bt)
    open(feat, "wb").write(ft)
    if not os.path.exists(a.gen_bam):
        os.makedirs(os.path.dirname(a.gen_bam), exist_ok=True)
        subprocess.check_call(["gcc", "-O2", "-o", a.gen_bam, os.path.join(ROOT, "tools", "gen_bam.c"), "-lz", "-lpthread"])
    jobs = [("parent summary-only", base, ["--summary-only"]), ("this summary-only", fastf, ["--summary-only"]),
            ("parent matrices", base, []), ("this matrices", fastf, []),
            ("this summary-only --neighbors", fastf, ["--summary-only", "--neighbors"]),
            ("this matrices --neighbors", fastf, ["--neighbors"])]
    times, stages = {j[0]: [] for j in jobs}, {}
    try:
        subprocess.check_call([a.gen_bam, bam, bar, feat, str(a.records), "7", "12", "91", "16"], stdout=subprocess.DEVNULL)
        lines = ["%d records, BAM %.2f GB, grid %s x %s, %d interleaved runs each, process start to exit" %
                 (a.records, os.path.getsize(bam) / 1e9, a.cells, a.depths, a.runs)]
        for _ in range(a.runs):
            for label, binary, extra in jobs:
                shutil.rmtree(od, ignore_errors=True)
                t = time.time()
                p = subprocess.run([binary, "sweep", "-b", bam, "-a", bar, "-f", feat, "-o", od, "-c", a.cells, "-r", a.depths] + extra,
                                   capture_output=True, text=True, env=dict(os.environ, FASTF_PROFILE="1"), timeout=900)
                times[label].append(time.time() - t)
                if p.returncode:
                    print(label + " failed\n" + p.stderr)
                    return 1
                stages[label] = [ln for ln in p.stderr.split("\n") if ln.startswith("[sweep] lists") or ln.startswith("[sweep] --neighbors")]
        for label, _, _ in jobs:
            v = times[label]
            lines.append("%-36s runs %s  median %.3f  spread %.3f" % (label, " ".join("%.3f" % x for x in v), statistics.median(v), max(v) - min(v)))
        for label, _, extra in jobs:
            if "--neighbors" in extra:
                lines += ["---- stage lines, " + label + " (last run)"] + stages[label]
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    open(os.path.join(a.out, "sweep_neighbors_%dM.txt" % (a.records // 1_000_000)), "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
