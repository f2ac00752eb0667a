"""filter throughput: reads/s to process exit of `fastF filter` on a 10x-shaped triple (R1 28 bp, I1 10 bp, R2 90 bp) as plain
text, gzip (concatenated members, the zlib streaming path) and BGZF (the parallel host inflate), with a 10x-sized whitelist
(6.8 M 16-mers) and a Cell Ranger barcodes.tsv (10 000 cells, "-1" suffix), and the FASTF_PROFILE stage times.  One framing's
files exist at a time.

    python tools/filter_bench.py --reads 20000000 --out profiles/filter_notes
"""
import argparse
import concurrent.futures as cf
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fastf_amd import synth  # noqa: E402


def gz_member(b):
    c = zlib.compressobj(1, zlib.DEFLATED, 31)
    return c.compress(b) + c.flush()


def chunks(text, size):
    return [text[o:o + size] for o in range(0, len(text), size)]


def run(cmd, env=None, timeout=3600):
    e = dict(os.environ)
    e.update(env or {})
    t = time.time()
    p = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=timeout)
    return time.time() - t, p


def write_framing(path, text, fmt, ex):
    with open(path, "wb") as f:
        if fmt == "plain":
            f.write(text)
        elif fmt == "gzip":
            for m in ex.map(gz_member, chunks(text, 64 << 20)):
                f.write(m)
        else:
            for m in ex.map(synth._bgzf_block, chunks(text, 0xff00), chunksize=256):
                f.write(m)
            f.write(synth._bgzf_block(b""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--rate", type=float, default=0.5)
    ap.add_argument("--framings", default="plain,bgzf,gzip")
    ap.add_argument("--dir", default="/tmp/filter_bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_notes"))
    a = ap.parse_args()
    from filter_ref import tenx_triple
    os.makedirs(a.dir, exist_ok=True)
    os.makedirs(a.out, exist_ok=True)
    t0 = time.time()
    parts = {"I1": [], "R1": [], "R2": []}
    pool = None
    step = 2_000_000
    for o in range(0, a.reads, step):
        tx, pl = tenx_triple(min(step, a.reads - o), seed=1, n_cells=a.cells, p_other=0.1)
        pool = pl
        for k in parts:
            parts[k].append(tx[k])
    texts = {k: b"".join(v) for k, v in parts.items()}
    del parts
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    big = acgt[rng.integers(0, 4, size=(6_800_000, 16))]
    nl = np.full((big.shape[0], 1), ord("\n"), dtype=np.uint8)
    wl_10x = np.concatenate([big, nl], axis=1).tobytes() + b"".join(b + b"\n" for b in pool)
    wl_tsv = b"".join(b + b"-1\n" for b in pool)
    wls = {"10x": os.path.join(a.dir, "3M-february-2018.txt"), "tsv": os.path.join(a.dir, "barcodes.tsv")}
    open(wls["10x"], "wb").write(wl_10x)
    open(wls["tsv"], "wb").write(wl_tsv)
    print("generated %d reads (%.1f GB of text) in %.1f s" % (a.reads, sum(len(t) for t in texts.values()) / 1e9, time.time() - t0),
          flush=True)
    fastf = os.path.join(ROOT, "fastf_amd", "bin", "fastF")
    outs = {}
    rc = 0
    with cf.ProcessPoolExecutor(16) as ex:
        for fmt in a.framings.split(","):
            files = {k: os.path.join(a.dir, "%s.%s" % (k, fmt)) for k in texts}
            for k in texts:
                write_framing(files[k], texts[k], fmt, ex)
            for wk in ("10x", "tsv"):
                od = os.path.join(a.dir, "o_%s_%s" % (fmt, wk))
                os.makedirs(od, exist_ok=True)
                cmd = [fastf, "filter", "-I", files["I1"], "-R", files["R1"], "-r", files["R2"], "-o", od, "-w", wls[wk],
                       "-t", str(a.rate)]
                dt, p = run(cmd, {"FASTF_PROFILE": "1"})
                if p.returncode:
                    print(p.stderr)
                    return 1
                sizes = {k: os.path.getsize(os.path.join(od, "%s.fastq.gz" % k)) for k in texts}
                outs[(fmt, wk)] = sizes["R1"]
                line = "%s, whitelist %s: %d reads, inputs %.2f GB, %.3f s to exit = %.2f M reads/s; outputs %s\n%s" % (
                    fmt, wk, a.reads, sum(os.path.getsize(f) for f in files.values()) / 1e9, dt, a.reads / dt / 1e6,
                    " ".join("%s %.1f MB" % (k, v / 1e6) for k, v in sizes.items()), p.stderr)
                print(line, flush=True)
                with open(os.path.join(a.out, "filter_%s_%s.txt" % (fmt, wk)), "w") as f:
                    f.write(line)
                for k in texts:
                    os.remove(os.path.join(od, "%s.fastq.gz" % k))
            for f in files.values():
                os.remove(f)
    return rc


if __name__ == "__main__":
    sys.exit(main())
