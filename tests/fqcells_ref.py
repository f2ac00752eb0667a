"""The definition of `fastF fqcells` (include/fastf_amd.h) in plain Python, for tests/test_fqcells_host.py and
tests/test_gpu_fqcells.py: a dict over the reads, a sort for the order, the three rules; the per-barcode reduce of a sorted key
table; and the hand-built fixtures both files use.

`defect` turns one rule into a wrong one (DEFECTS); tests/test_fqcells_host.py shows that every one of them changes what some
fixture of the GPU tests expects, so that the device tests would fail for these bugs."""
import collections
import functools
import itertools

import numpy as np

import filter_ref as R

TAG = 1 << 63
ACGT = b"ACGT"
HEADER = b"barcode\treads\tumis\trank\tcalled\n"
SUMMARY_HEADER = b"reads\tcounted\tother\tbarcodes\tumis\trule\targ\tthreshold\tcalled\tcalled_reads\tcalled_umis\n"

DEFECTS = (
    "n_in_umi_counted",        # a read with N in its UMI (the barcode clean) is still counted
    "tile_split_twice",        # a barcode whose UMI run crosses a tile boundary of the reduce starts a second row there
    "tie_reads_ascending",     # equal umis: the fewer reads rank first
    "e_truncated",             # -e: T = m / 10, not (m + 5) / 10
    "rank_off_by_one",         # -e: m read at rank min(B, E / 100 + 1) + 1
    "k_keeps_ties",            # -k: every barcode tied (umis and reads) with the K-th is called too
)


# ---------------------------------------------------------------- the definition
def pack(b):
    v = 0
    for c in b:
        v = (v << 2) | ACGT.index(c)
    return v


def unpack(v, n):
    return bytes(ACGT[(v >> (2 * (n - 1 - i))) & 3] for i in range(n))


def read_table(text, l, u, defect=None):
    """(n_reads, other, {barcode bytes: (reads, umis)}) of an R1 text"""
    lines = R.lines(text)
    n_reads = (len(lines) + 3) // 4
    per = collections.defaultdict(collections.Counter)
    other = 0
    for i in range(n_reads):
        seq = lines[4 * i + 1] if 4 * i + 1 < len(lines) else b""
        key = seq[:l + u]
        clean = key[:l] if defect == "n_in_umi_counted" else key
        if len(key) == l + u and all(c in ACGT for c in clean):
            per[key[:l]][key[l:]] += 1
        else:
            other += 1
    return n_reads, other, {b: (sum(c.values()), len(c)) for b, c in per.items()}


def call(rows, rule, arg, defect=None):
    """rows: [(barcode, reads, umis)] with distinct barcodes that compare as their bytes do (bytes or packed ints).
    Returns ({barcode: rank}, {barcode: called}, threshold)"""
    assert rule in "ekm" and arg >= 1
    tie = (lambda r: r[1]) if defect == "tie_reads_ascending" else (lambda r: -r[1])
    order = sorted(rows, key=lambda r: (-r[2], tie(r), r[0]))
    B = len(order)
    rank = {r[0]: k + 1 for k, r in enumerate(order)}
    if rule == "k":
        K = min(arg, B)
        thr = order[K - 1][2] if B else 0
        last = order[K - 1] if B else None
        called = {r[0]: rank[r[0]] <= K or (defect == "k_keeps_ties" and r[1:] == last[1:]) for r in order}
    else:
        if rule == "m":
            thr = arg
        else:
            at = min(B, arg // 100 + 1)
            if defect == "rank_off_by_one":
                at = min(B, at + 1)
            m = order[at - 1][2] if B else 0
            thr = max(1, m // 10 if defect == "e_truncated" else (m + 5) // 10)
        called = {r[0]: r[2] >= thr for r in order}
    return rank, called, thr


def outputs(n_reads, other, rows, l, rule, arg, defect=None):
    """the bytes of the three files for rows [(barcode bytes, reads, umis)]"""
    rank, called, thr = call(rows, rule, arg, defect)
    rows = sorted(rows)
    tsv = HEADER + b"".join(b"%s\t%d\t%d\t%d\t%d\n" % (b, r, m, rank[b], called[b]) for b, r, m in rows)
    wl = b"".join(b + b"\n" for b, _, _ in rows if called[b])
    yes = [r for r in rows if called[r[0]]]
    s = dict(reads=n_reads, counted=n_reads - other, other=other, barcodes=len(rows), umis=sum(r[2] for r in rows), rule=rule, arg=arg,
             threshold=thr, called=len(yes), called_reads=sum(r[1] for r in yes), called_umis=sum(r[2] for r in yes))
    summary = SUMMARY_HEADER + b"%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\n" % (
        s["reads"], s["counted"], s["other"], s["barcodes"], s["umis"], rule.encode(), arg, thr, s["called"], s["called_reads"],
        s["called_umis"])
    return dict(tsv=tsv, whitelist=wl, summary=summary, dict=s)


def py_fqcells(text, l=16, u=10, rule="e", arg=3000, defect=None):
    n_reads, other, per = read_table(text, l, u, defect)
    return outputs(n_reads, other, [(b, r, m) for b, (r, m) in per.items()], l, rule, arg, defect)


def reduce_ref(keys, counts, u, tile=None, defect=None):
    """rows (barcode = key without its tag bit >> 2u, reads, umis) of m1 ascending keys, as lists"""
    bc, reads, umis = [], [], []
    prev = None
    for i, (k, c) in enumerate(zip(keys, counts)):
        b = (int(k) & (TAG - 1)) >> (2 * u)
        if b != prev or (defect == "tile_split_twice" and tile and i % tile == 0):
            bc.append(b), reads.append(0), umis.append(0)
        reads[-1] += int(c)
        umis[-1] += 1
        prev = b
    return bc, reads, umis


# ---------------------------------------------------------------- seam fixtures: hand-built sorted tables
def keys_of_runs(runs, l, u, top=False):
    """ascending DNA-form keys: run k is one barcode with runs[k] ascending UMIs; top: the barcodes end at the highest one"""
    assert l >= 1 and l + u <= 31 and all(1 <= n <= 4 ** u for n in runs)
    step = 3 if 3 * (len(runs) + 1) < 4 ** l else 1
    first = 4 ** l - 1 - step * (len(runs) - 1) if top else 1
    assert first >= 0 and first + step * (len(runs) - 1) < 4 ** l
    out = []
    for k, n in enumerate(runs):
        bc = first + step * k
        gap = max(1, (4 ** u - 1) // max(n, 1)) if u else 1
        out += [TAG | (bc << (2 * u)) | (j * gap if n > 1 else (7 * k) % 4 ** u) for j in range(n)]
    assert all(a < b for a, b in zip(out, out[1:]))
    return np.array(out, dtype=np.uint64)


def cut_runs(m1, lengths):
    """run lengths cycling through `lengths` that add up to m1"""
    runs, it = [], itertools.cycle(lengths)
    while sum(runs) < m1:
        runs.append(min(next(it), m1 - sum(runs)))
    return runs


def seam_sizes(T):
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7]


def seam_fixtures(T):
    """[(name, keys uint64, counts uint32, len_umi)]: every size with every pattern that fits it"""
    fx = []
    for m1 in seam_sizes(T):
        rng = np.random.default_rng(m1)
        cnt = lambda n=m1: rng.integers(1, 50, size=n).astype(np.uint32)  # noqa: E731
        if m1 == 0:
            fx.append(("empty", np.zeros(0, np.uint64), np.zeros(0, np.uint32), 10))
            continue
        fx.append(("one_barcode m1=%d" % m1, keys_of_runs([m1], 16, 10), cnt(), 10))
        fx.append(("each_its_own m1=%d" % m1, keys_of_runs([1] * m1, 16, 10), cnt(), 10))
        fx.append(("runs_1_2 m1=%d" % m1, keys_of_runs(cut_runs(m1, [1, 2]), 16, 10), cnt(), 10))
        fx.append(("u=0 m1=%d" % m1, keys_of_runs([1] * m1, 16, 0), cnt(), 0))
        fx.append(("u=1 m1=%d" % m1, keys_of_runs(cut_runs(m1, [4, 1, 3, 2]), 16, 1), cnt(), 1))
        fx.append(("u=15 l+u=31 m1=%d" % m1, keys_of_runs(cut_runs(m1, [1, 5, 2, 70]), 16, 15, top=True), cnt(), 15))
        if m1 > T:                                           # a run on the last key of a tile and the first of the next, singles around
            fx.append(("straddle m1=%d" % m1, keys_of_runs([1] * (T - 1) + [2] + [1] * (m1 - T - 1), 16, 10), cnt(), 10))
        if m1 >= 3 * T:                                      # more than two whole tiles in one run, short runs on both sides
            head, tail = [1, 2, 1], cut_runs(m1 - 4 - (2 * T + T // 2), [2, 1, 3])
            fx.append(("long_run m1=%d" % m1, keys_of_runs(head + [2 * T + T // 2] + tail, 16, 10), cnt(), 10))
        if m1 >= 63:                                         # reads[] needs 64 bits
            c = cnt()
            c[m1 // 2 - 1:m1 // 2 + 2] = 0xffffffff
            fx.append(("wide_counts m1=%d" % m1, keys_of_runs(cut_runs(m1, [m1 // 2 - 3, 9, m1]), 16, 10), c, 10))
    return fx


# ---------------------------------------------------------------- end-to-end fixtures: FASTQ text
def _bc(k, l=16):
    return unpack((k * 2654435761 + 12345) % 4 ** l, l)


def _umi(k, u=10):
    return unpack((k * 40503 + 7) % 4 ** u, u)


@functools.lru_cache(maxsize=None)
def fastq_fixture(l=16, u=10, seed=3):
    """R1 text of a few thousand reads, shuffled:
      16 cells of 89, 86, .. 44 UMIs (1 to 3 reads a UMI); two cells tied at 30 UMIs and 60 reads; barcodes of 8, 7, 6 and 5
      UMIs (the thresholds' neighbours); 250 background barcodes of 1 to 3 UMIs and 1 or 2 reads a UMI (ties on umis with
      different reads); and reads that are not counted: N in the barcode, N in the UMI, a short line, CR LF lines whose CR falls
      inside the first l + u bytes, lower case.  One CR LF read whose first l + u bytes are clean is counted, as the definition says."""
    rng = np.random.default_rng(seed)
    seqs = []
    plan = [(44 + 3 * c, None) for c in range(16)] + [(30, 2), (30, 2), (8, 1), (7, 1), (6, 2), (5, 1)]
    plan += [(1 + k % 3, 1 + k % 2) for k in range(250)]
    for k, (n_umi, copies) in enumerate(plan):
        for j in range(n_umi):
            n = copies if copies else 1 + (k + j) % 3
            seqs += [_bc(k, l) + _umi(1000 * k + j, u) + b"TTTTGGGG\n"] * n
    good = _bc(0, l) + _umi(0, u)
    bad = [b"N" + good[1:] + b"TT\n", good[:l] + b"N" + good[l + 1:] + b"TT\n", good[:l + u - 1] + b"N\n", good[:10] + b"\n", b"\n",
           good[:l + u - 1] + b"\r\n", good.lower() + b"TT\n", good[:l + u - 1] + b"a" + b"TT\n"]
    seqs += bad * 6 + [good + b"\r\n"]
    order = rng.permutation(len(seqs))
    recs = []
    for i, q in enumerate(order):
        s = seqs[q]
        eol = b"\r\n" if s.endswith(b"\r\n") else b"\n"
        recs.append(b"@read%d" % i + eol + s + b"+" + eol + b"F" * (len(s) - len(eol)) + eol)
    return b"".join(recs)


@functools.lru_cache(maxsize=None)
def tie_rank(l=16, u=10):
    """K such that the barcodes at ranks K and K + 1 of fastq_fixture tie on umis and reads"""
    _, _, per = read_table(fastq_fixture(l, u), l, u)
    order = sorted(((b, r, m) for b, (r, m) in per.items()), key=lambda r: (-r[2], -r[1], r[0]))
    ks = [k + 1 for k in range(len(order) - 1) if order[k][1:] == order[k + 1][1:] and order[k][2] > 3]
    assert ks
    return ks[0]


def e2e_cases():
    """[(name, text, l, u, rule, arg)] the GPU tests run through the CLI against py_fqcells"""
    t = fastq_fixture()
    uncounted = b"".join(b"@x%d\nACGTNACGTACGTACGTACGTACGTACGT\n+\nFFFFFFFFFFFFFFFFFFFFFFFFFFFFF\n" % i for i in range(40)) + b"@y\nAC\n+\nFF\n"
    return [
        ("default_e3000", t, 16, 10, "e", 3000),
        ("e1100_rounds_up", t, 16, 10, "e", 1100),
        ("e_beyond_B", t, 16, 10, "e", 10 ** 6),
        ("k_at_a_tie", t, 16, 10, "k", tie_rank()),
        ("k_beyond_B", t, 16, 10, "k", 10 ** 9),
        ("m8", t, 16, 10, "m", 8),
        ("u0_by_reads", t, 16, 0, "k", 5),
        ("l12_u14", t, 12, 14, "m", 2),
        ("no_counted_read", uncounted, 16, 10, "e", 3000),
        ("last_line_open", t[:-1], 16, 10, "m", 6),
    ]
