"""freq throughput: reads/s to process exit of `fastF freq` on a 10x-shaped R1 (~115 bytes per read) as plain text, gzip
(concatenated members, the zlib streaming path) and BGZF (the parallel host inflate), with FASTF_PROFILE stage times; the
reference CLI (oracle/_ref/fastF_refmain, single-threaded) on a cut of the same reads as the reference line.

    python tools/freq_bench.py --reads 20000000 --ref-reads 2000000 --out profiles/r7_notes
"""
import argparse
import concurrent.futures as cf
import os
import subprocess
import sys
import time
import zlib

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--ref-reads", type=int, default=2_000_000)
    ap.add_argument("--dir", default="/tmp/freq_bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7_notes"))
    a = ap.parse_args()
    from test_gpu_freq import tenx_text
    os.makedirs(a.dir, exist_ok=True)
    os.makedirs(a.out, exist_ok=True)
    text = b"".join(tenx_text(min(2_000_000, a.reads - o), seed=100 + o // 2_000_000) for o in range(0, a.reads, 2_000_000))
    files = {"plain": os.path.join(a.dir, "r1.fq"), "gzip": os.path.join(a.dir, "r1.fq.gz"), "bgzf": os.path.join(a.dir, "r1.bgzf.fq.gz")}
    with open(files["plain"], "wb") as f:
        f.write(text)
    with cf.ProcessPoolExecutor(16) as ex:
        with open(files["gzip"], "wb") as f:
            for m in ex.map(gz_member, chunks(text, 64 << 20)):
                f.write(m)
        with open(files["bgzf"], "wb") as f:
            for m in ex.map(synth._bgzf_block, chunks(text, 0xff00), chunksize=256):
                f.write(m)
            f.write(synth._bgzf_block(b""))
    cut = os.path.join(a.dir, "r1.cut.fq")
    with open(cut, "wb") as f:
        f.write(text[:text.index(b"@", len(text) * a.ref_reads // a.reads) if a.ref_reads < a.reads else len(text)])
    del text
    fastf = os.path.join(ROOT, "fastf_amd", "bin", "fastF")
    refmain = os.path.join(ROOT, "oracle", "_ref", "fastF_refmain")
    lines = []
    for fmt in ("plain", "gzip", "bgzf"):
        od = os.path.join(a.dir, "o_" + fmt)
        os.makedirs(od, exist_ok=True)
        run([fastf, "freq", "-R", files[fmt], "-o", od])                       # warm: page cache, code objects
        dt, p = run([fastf, "freq", "-R", files[fmt], "-o", od], {"FASTF_PROFILE": "1"})
        if p.returncode:
            print(p.stderr)
            return 1
        line = "%s: %d reads, %.1f MB file, %.3f s to exit = %.1f M reads/s\n%s" % (
            fmt, a.reads, os.path.getsize(files[fmt]) / 1e6, dt, a.reads / dt / 1e6, p.stderr)
        print(line)
        lines.append(line)
        with open(os.path.join(a.out, "freq_%s.txt" % fmt), "w") as f:
            f.write(line)
    outs = [open(os.path.join(a.dir, "o_" + f, "whitelist.txt"), "rb").read() for f in ("plain", "gzip", "bgzf")]
    same = outs[0] == outs[1] == outs[2]
    print("outputs identical across framings:", same)
    if os.path.exists(refmain):
        od = os.path.join(a.dir, "o_ref")
        os.makedirs(od, exist_ok=True)
        dt, p = run([refmain, "freq", "-R", cut, "-o", od], {"OMP_NUM_THREADS": "1"})
        line = "reference fastF_refmain freq, plain text, %d reads: %.3f s = %.2f M reads/s (rc %d)\n" % (a.ref_reads, dt, a.ref_reads / dt / 1e6, p.returncode)
        od2 = os.path.join(a.dir, "o_cut")
        os.makedirs(od2, exist_ok=True)
        dt2, p2 = run([fastf, "freq", "-R", cut, "-o", od2])
        line += "fastF freq on the same cut: %.3f s; same bytes: %s\n" % (
            dt2, open(os.path.join(od, "whitelist.txt"), "rb").read() == open(os.path.join(od2, "whitelist.txt"), "rb").read())
        print(line)
        with open(os.path.join(a.out, "freq_ref.txt"), "w") as f:
            f.write(line)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
