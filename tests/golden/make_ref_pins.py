"""Generates tests/golden/ref_pins.json: what the REFERENCE's own code answers to the inputs of the pins in
tests/test_oracle_pins.py (mt19937ar.c, utils.c SampleInt, compiled in place into oracle/_ref/libfastf_ref.so),
tests/test_oracle_tag_pins.py (filter.c's tree code, oracle/_ref/libfastf_ref_tree.so) and tests/test_ref_main_link.py
(the reference's main.c + argparse.c linked against the product library, oracle/_ref/fastF_refmain), so that those pins
also hold where the reference sources are absent.
Run after build() on a machine that has the reference sources:  python tests/golden/make_ref_pins.py"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "ref_pins.json")
if not os.path.exists(OUT):            # (the test modules below read it at import: a first run starts from an empty one)
    json.dump({"cli": {}}, open(OUT, "w"))
from oracle import oracle as O  # noqa: E402
import test_oracle_pins as P  # noqa: E402
import test_oracle_tag_pins as T  # noqa: E402
import test_ref_main_link as M  # noqa: E402

ref, R = O.ref_lib(), O.ref_tree_lib()
assert ref is not None and R is not None and os.path.exists(M.REFMAIN), "build oracle/_ref first (build() with the reference present)"
out = {"mt": {}, "sample_int": [], "tag_tree": [], "crb_rows": {}, "cli": {}}

for seed in P.MT_SEEDS:
    ref.init_genrand(seed)
    ints = [ref.genrand_int32() & 0xFFFFFFFF for _ in range(2000)]
    ref.init_genrand(seed)
    out["mt"][str(seed)] = {"genrand_int32": ints, "genrand_real1": [ref.genrand_real1() for _ in range(100)]}

for n, k, seed in P.SAMPLE_INT_CASES:
    seq = ref.GetSeqInt(0, n - 1, 1)
    got = ref.SampleInt(seq, n, k, 0, seed)
    out["sample_int"].append({"n": n, "k": k, "seed": seed, "sorted": sorted(got[i] for i in range(k)),
                              "next_genrand_int32": ref.genrand_int32() & 0xFFFFFFFF})

for seed, n, pool in T.TREE_CASES:
    tags = T._random_tags(np.random.default_rng(seed), n, pool)
    out["tag_tree"].append({"seed": seed, "n": n, "pool": pool, "print_tree": T._ref_print_tree(R, tags).decode()})

cbs, crs = T._crb_case()
out["crb_rows"] = {"same_row": {cb.decode(): T._ref_same_row(R, [crs[i] for i in range(len(cbs)) if cbs[i] == cb]).decode()
                                for cb in sorted(set(cbs))},
                   "cb_print_tree": T._ref_print_tree(R, cbs).decode()}

with tempfile.TemporaryDirectory() as d:
    bam, tsv = os.path.join(d, "e.bam"), os.path.join(d, "e.tsv")
    open(bam, "wb").close()
    open(tsv, "wb").close()
    for args in M.BAD_ARGS:
        p = subprocess.run([M.REFMAIN, "bam2db"] + [a.format(bam=bam, tsv=tsv) for a in args], capture_output=True, text=True)
        first = p.stderr.splitlines()[:1]
        out["cli"][M.case_id(args)] = {"returncode": p.returncode,
                                       "stderr_first_line": [ln.replace(bam, "{bam}").replace(tsv, "{tsv}") for ln in first]}

json.dump(out, open(OUT, "w"), separators=(",", ":"))
print("wrote ref_pins.json")
