"""fqcells against freq: seconds to process exit of `fastF fqcells -l 16 -u 10` and of `fastF freq -l 16 -u 10` (this tree's, and
another build's with --parent) on the 10x-shaped R1 of tools/freq_bench.py, plain and BGZF, with the FASTF_PROFILE stage lines.
The runs are interleaved and the order of the commands rotates from repeat to repeat, so that each follows each.  Checks at
size: freq's whitelist.txt of the two builds byte for byte, and fqcells' rows against freq's rows regrouped by barcode.
--startup N: the commands N times each, alternating, on a 1000-read file — the open stage (HIP runtime + histogram) with
nothing else to wait for.  --parent-lib: bench.py with this tree's library and with that one.

    python tools/fqcells_bench.py --reads 20000000 --runs 3 --startup 8 --parent /path/to/parent/bin/fastF \\
        --parent-lib /path/to/parent/lib/libfastf_amd.so --out profiles/fqcells_notes
"""
import argparse
import concurrent.futures as cf
import gzip
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fastf_amd import synth  # noqa: E402

THIS = os.path.join(ROOT, "fastf_amd", "bin", "fastF")
LOG = None


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    LOG.write(s + "\n")
    LOG.flush()


def step(cmd, env=None, limit=600):
    e = dict(os.environ, FASTF_PROFILE="1")
    e.update(env or {})
    t = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=e)
    dt = time.time() - t
    if p.returncode != 0:
        say("FAILED rc=%d: %s\n%s\n%s" % (p.returncode, " ".join(os.path.basename(c) for c in cmd), p.stdout[-2000:], p.stderr[-4000:]))
        sys.exit(1)
    return dt, p


def open_stage(p):
    m = re.search(r"open \(HIP runtime \+ histogram\) ([0-9.]+) s", p.stderr)
    return float(m.group(1)) if m else float("nan")


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--startup", type=int, default=0)
    ap.add_argument("--parent", default=None, help="fastF of another build (the parent commit's): its freq is timed too")
    ap.add_argument("--parent-lib", default=None, help="libfastf_amd.so of that build: bench.py runs with it and with this tree's")
    ap.add_argument("--dir", default="/tmp/fqcells_bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fqcells_notes"))
    a = ap.parse_args()
    from test_gpu_freq import tenx_text
    os.makedirs(a.dir, exist_ok=True)
    os.makedirs(a.out, exist_ok=True)
    LOG = open(os.path.join(a.out, "fqcells_vs_freq_%dM.txt" % (a.reads // 1_000_000)), "w")
    runs = [("this freq", [THIS, "freq"], "o_this"), ("this fqcells", [THIS, "fqcells"], "o_cells")]
    if a.parent:
        runs.insert(0, ("parent freq", [a.parent, "freq"], "o_parent"))
    for _, _, d in runs:
        os.makedirs(os.path.join(a.dir, d), exist_ok=True)

    if a.startup:
        tiny = os.path.join(a.dir, "tiny.fq")
        with open(tiny, "wb") as f:
            f.write(tenx_text(1000, seed=1))
        opens = {n: [] for n, _, _ in runs}
        walls = {n: [] for n, _, _ in runs}
        for rep in range(a.startup):
            for name, cmd, od in runs[rep % len(runs):] + runs[:rep % len(runs)]:
                dt, p = step(cmd + ["-R", tiny, "-o", os.path.join(a.dir, od), "-l", "16", "-u", "10"])
                opens[name].append(open_stage(p))
                walls[name].append(dt)
        for name in opens:
            say("== startup, 1000 reads, %-13s open stage %s | to exit %s" % (
                name, " ".join("%.3f" % x for x in opens[name]), " ".join("%.3f" % x for x in walls[name])))

    t = time.time()
    text = b"".join(tenx_text(min(2_000_000, a.reads - o), seed=100 + o // 2_000_000) for o in range(0, a.reads, 2_000_000))
    files = {"plain": os.path.join(a.dir, "r1.fq"), "bgzf": os.path.join(a.dir, "r1.bgzf.fq.gz")}
    with open(files["plain"], "wb") as f:
        f.write(text)
    with cf.ProcessPoolExecutor(16) as ex, open(files["bgzf"], "wb") as f:
        for m in ex.map(synth._bgzf_block, [text[o:o + 0xff00] for o in range(0, len(text), 0xff00)], chunksize=256):
            f.write(m)
        f.write(synth._bgzf_block(b""))
    say("generated %d reads: %d bytes of text, %d bytes of BGZF, %.1f s" % (a.reads, len(text), os.path.getsize(files["bgzf"]), time.time() - t))
    del text
    for fmt, path in files.items():
        times = {n: [] for n, _, _ in runs}
        for rep in range(a.runs):
            for name, cmd, od in runs[rep % len(runs):] + runs[:rep % len(runs)]:
                dt, p = step(cmd + ["-R", path, "-o", os.path.join(a.dir, od), "-l", "16", "-u", "10"])
                times[name].append(dt)
                say("[%s rep %d] %-13s %.3f s" % (fmt, rep, name, dt))
                for ln in (p.stdout + p.stderr).splitlines():
                    if ln.startswith("[") or ln.startswith("fqcells:"):
                        say("    " + ln)
        for name, ts in times.items():
            say("== %s %-13s best %.3f s, runs %s" % (fmt, name, min(ts), " ".join("%.3f" % x for x in ts)))
        rows_freq = open(os.path.join(a.dir, "o_this", "whitelist.txt"), "rb").read()
        if a.parent:
            same = open(os.path.join(a.dir, "o_parent", "whitelist.txt"), "rb").read() == rows_freq
            say("== %s freq whitelist.txt parent == this: %s (%d bytes)" % (fmt, same, len(rows_freq)))
        per = {}                                             # freq's DNA-form rows regrouped: barcode -> [reads, umis]
        for ln in rows_freq.split(b"\n"):
            k, _, c = ln.rpartition(b",")
            if len(k) == 26 and set(k) <= set(b"ACGT"):
                r = per.setdefault(k[:16], [0, 0])
                r[0] += int(c)
                r[1] += 1
        rows = gzip.decompress(open(os.path.join(a.dir, "o_cells", "fqcells.tsv.gz"), "rb").read()).split(b"\n")[1:-1]
        got = {r.split(b"\t")[0]: [int(r.split(b"\t")[1]), int(r.split(b"\t")[2])] for r in rows}
        say("== %s fqcells rows == freq's rows regrouped: %s (%d barcodes)" % (fmt, got == per, len(got)))
        say("    " + open(os.path.join(a.dir, "o_cells", "fqcells_summary.tsv")).read().replace("\n", "\n    "))
    if a.parent_lib:
        for name, env in (("this tree", {}), ("parent library", {"FASTF_LIB_OVERRIDE": a.parent_lib}), ("this tree again", {})):
            dt, p = step([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3"], env)
            ms = re.search(r'"ms_per_step": ([0-9.]+)', p.stdout)
            say("bench.py (%s): %s ms per step" % (name, ms.group(1) if ms else "?"))


if __name__ == "__main__":
    main()
