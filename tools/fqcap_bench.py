"""fqcap against filter: seconds to process exit of `fastF fqcap -n <median h>` and of `fastF filter -t 0.5` (this tree's, and
another build's with --parent) on the same 10x-shaped triple (R1 28 bp, I1 10 bp, R2 90 bp) with a Cell Ranger barcodes.tsv as
the whitelist, runs interleaved, with the FASTF_PROFILE stage times.  The cost expected of fqcap is one more read (and inflate)
of R1 on top of filter.

    python tools/fqcap_bench.py --reads 20000000 --framing plain --runs 3 --parent /path/to/parent/bin/fastF --out profiles/fqcap_notes
"""
import argparse
import concurrent.futures as cf
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from filter_bench import run, write_framing  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--rate", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--framing", default="plain")
    ap.add_argument("--parent", default=None, help="fastF of another build (the parent commit's): its filter is timed too")
    ap.add_argument("--dir", default="/tmp/fqcap_bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fqcap_notes"))
    a = ap.parse_args()
    from filter_ref import tenx_triple
    os.makedirs(a.dir, exist_ok=True)
    os.makedirs(a.out, exist_ok=True)
    parts = {"I1": [], "R1": [], "R2": []}
    step = 2_000_000
    for o in range(0, a.reads, step):
        tx, pool = tenx_triple(min(step, a.reads - o), seed=1, n_cells=a.cells, p_other=0.1)
        for k in parts:
            parts[k].append(tx[k])
    texts = {k: b"".join(v) for k, v in parts.items()}
    del parts
    wl = os.path.join(a.dir, "barcodes.tsv")
    open(wl, "wb").write(b"".join(b + b"-1\n" for b in pool))
    files = {k: os.path.join(a.dir, "%s.%s" % (k, a.framing)) for k in texts}
    with cf.ProcessPoolExecutor(16) as ex:
        for k in texts:
            write_framing(files[k], texts[k], a.framing, ex)
    del texts
    fastf = os.path.join(ROOT, "fastf_amd", "bin", "fastF")
    od = os.path.join(a.dir, "out")
    os.makedirs(od, exist_ok=True)
    io = ["-I", files["I1"], "-R", files["R1"], "-r", files["R2"], "-o", od, "-w", wl]
    # the median h of the matched cells: one untimed run with a cap nothing reaches
    _, p = run([fastf, "fqcap"] + io + ["-n", str(10 ** 9)])
    if p.returncode:
        print(p.stderr)
        return 1
    import gzip
    hs = [int(ln.split(b"\t")[1]) for ln in gzip.open(os.path.join(od, "fqcap_cells.tsv.gz")).read().split(b"\n")[1:-1]]
    cap = int(statistics.median(hs))
    legs = {"fqcap": [fastf, "fqcap"] + io + ["-n", str(cap)], "filter": [fastf, "filter"] + io + ["-t", str(a.rate)]}
    if a.parent:
        legs["filter (parent)"] = [a.parent, "filter"] + io + ["-t", str(a.rate)]
    times = {k: [] for k in legs}
    notes = {}
    for _ in range(a.runs):
        for k, cmd in legs.items():
            dt, p = run(cmd, {"FASTF_PROFILE": "1"})
            if p.returncode:
                print(p.stderr)
                return 1
            times[k].append(dt)
            notes[k] = (p.stdout.strip().split("\n")[-1] if k == "fqcap" else "") + "\n" + p.stderr.strip()
    lines = ["%d reads, %d cells, framing %s, inputs %.2f GB, fqcap -n %d (median h of %d cells), filter -t %g, %d runs interleaved" % (
        a.reads, a.cells, a.framing, sum(os.path.getsize(f) for f in files.values()) / 1e9, cap, len(hs), a.rate, a.runs)]
    for k in legs:
        lines.append("%-16s %s s to exit (min %.3f, %.2f M reads/s)\n%s" % (
            k, " ".join("%.3f" % t for t in times[k]), min(times[k]), a.reads / min(times[k]) / 1e6, notes[k]))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(os.path.join(a.out, "fqcap_%s_tsv.txt" % a.framing), "w") as f:
        f.write(text)
    for f in list(files.values()) + [os.path.join(od, n) for n in os.listdir(od)]:
        os.remove(f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
