"""Reference and window builders for the device record stage (fastf_amd/csrc/gpu_records.hpp: gr_hop_kernel, gr_stitch_kernel,
gr_repair_kernel, gr_pack_kernel), in plain Python: the expectations of tests/test_gpu_record_windows.py, proved against the
project's host code in tests/test_grwin_ref_host.py.  Nothing here is imported from the library; the rules are restated from the
BAM format and from what gpu_records.hpp and host_io.c say about them.

Offsets are absolute offsets into the device's window buffer, as the kernels see them: `image(case)` is that buffer (`start`
bytes nobody reads, then the case's bytes).  A case is `(bytes, start, n_ref, end)`; its window is `[start, end)`, and whatever
`bytes` holds behind `end` is what the device buffer holds there too (stale bytes of an earlier window: case H, the G cuts).

`device(...)` runs hop, stitch, repair, stitch and the pack's index arithmetic as the kernels do and says what the API would
return; with `wrong=` one rule is replaced by a plausible mistake, to show on the CPU which cases see it."""
import functools
import struct
import zlib

import numpy as np

from fastf_amd.synth import bam_record, aux_Z, aux_int

GR_SEG = 32 << 10
GR_SEG_RECS = GR_SEG // 36 + 2
GR_STAGE_OVER = 4096
GR_PLAUSIBLE = 3
NONE = 2 ** 64 - 1
N_REF = 2

_u32 = struct.Struct("<I").unpack_from
_i32 = struct.Struct("<i").unpack_from
_u16 = struct.Struct("<H").unpack_from


# ---------------------------------------------------------------- the rules
def rec_end(buf, o, end):
    """offset just behind the record at o if a whole, structurally valid record lies in [o, end); 0 otherwise"""
    if end - o < 36:
        return 0
    bs = _u32(buf, o)[0]
    if bs < 32 or bs + 4 > end - o:
        return 0
    l_seq = _u32(buf, o + 20)[0]
    fixed = 32 + buf[o + 12] + 4 * _u16(buf, o + 16)[0] + (l_seq + 1) // 2 + l_seq
    return o + 4 + bs if fixed <= bs else 0


def rec_plausible(buf, o, end, n_ref):
    if not rec_end(buf, o, end):
        return False
    ref, pos = _i32(buf, o + 4)[0], _i32(buf, o + 8)[0]
    nref, npos = _i32(buf, o + 24)[0], _i32(buf, o + 28)[0]
    if ref < -1 or ref + 1 > n_ref or nref < -1 or nref + 1 > n_ref or pos < -1 or npos < -1:
        return False
    l_name = buf[o + 12]
    if l_name < 1 or buf[o + 36 + l_name - 1] != 0:
        return False
    return all(33 <= c <= 126 for c in buf[o + 36:o + 36 + l_name - 1])


def chain_meets_window_end(buf, q, end):
    if end - q < 36:
        return True
    bs = _u32(buf, q)[0]
    return 32 <= bs <= (64 << 20) and bs + 4 > end - q


def chain(buf, start, end):
    """(offsets of the complete records from `start`, the handover: offset behind the last of them)"""
    offs, o = [], start
    while True:
        e = rec_end(buf, o, end)
        if not e:
            return offs, o
        offs.append(o)
        o = e


def guess(buf, lo, hi, end, n_ref):
    """first offset in [lo, hi) from which three plausible records follow each other, or fewer that meet the window's end"""
    for o in range(lo, hi):
        q, k = o, 0
        while k < GR_PLAUSIBLE and rec_plausible(buf, q, end, n_ref):
            q = rec_end(buf, q, end)
            k += 1
        if k == GR_PLAUSIBLE or (k > 0 and chain_meets_window_end(buf, q, end)):
            return o
    return NONE


def n_segments(start, end):
    return (end - start + GR_SEG - 1) // GR_SEG


def seg_range(s, start, end):
    lo = start + s * GR_SEG
    return lo, min(lo + GR_SEG, end)


def hop(buf, start, end, n_ref, valid_end=None):
    """per segment (first, exit, n) and its record offsets, as gr_hop_kernel leaves them; valid_end: the bound the walk validates
    records against (the window's end; anything else is a mistake)"""
    vend = end if valid_end is None else valid_end
    segs, offs = [], []
    for s in range(n_segments(start, end)):
        lo, hi = seg_range(s, start, end)
        first = start if s == 0 else guess(buf, lo, hi, end, n_ref)
        if first == NONE:
            segs.append((NONE, lo, 0))
            offs.append([])
            continue
        o, l = first, []
        while o < hi:
            e = rec_end(buf, o, vend)
            if not e:
                break
            l.append(o)
            o = e
        segs.append((first, o, len(l)))
        offs.append(l)
    return segs, offs


def segments(buf, start, end, n_ref):
    return hop(buf, start, end, n_ref)[0]


def true_segments(buf, start, end):
    """(first, exit, n) of every segment on the true chain: what a segment holds once it is in step"""
    offs, hand = chain(buf, start, end)
    out, i, entry = [], 0, start
    for s in range(n_segments(start, end)):
        lo, hi = seg_range(s, start, end)
        j = i
        while j < len(offs) and offs[j] < hi:
            j += 1
        exit_ = offs[j] if j < len(offs) else hand
        out.append((entry, exit_, j - i))
        i, entry = j, exit_
    return out


def _bad(segs, idx, exits=None):
    if exits is not None:                                     # (wrong rule: a segment is judged by where its chain ends)
        return segs[idx][1] != exits[idx]
    return segs[idx][0] == NONE or segs[idx - 1][1] != segs[idx][0]


def repair(segs, buf, start, end, offs=None, one_only=False, exits=None):
    """the repair walk over the hop's table: (segments walked again, the table after it, the offsets after it)"""
    segs = list(segs)
    offs = [list(l) for l in offs] if offs is not None else [[] for _ in segs]
    n_seg, s, repaired = len(segs), 1, 0
    while s < n_seg:
        sb = next((i for i in range(s, min(s + 64, n_seg)) if _bad(segs, i, exits)), None)
        if sb is None:
            s += 64
            continue
        o = segs[sb - 1][1]
        while True:
            lo, hi = seg_range(sb, start, end)
            first, l = o, []
            while lo <= o < hi:
                e = rec_end(buf, o, end)
                if not e:
                    break
                l.append(o)
                o = e
            segs[sb], offs[sb] = (first, o, len(l)), l
            repaired += 1
            sb += 1
            if one_only or sb >= n_seg or segs[sb][0] == o:
                break
        s = sb + 1
    return repaired, segs, offs


def staged(buf, o, start, end):
    """gr_pack_kernel's choice for the record at o: (parsed from the staged bytes?, shift, record end minus want_end)"""
    s = (o - start) // GR_SEG
    lo = start + s * GR_SEG
    a0 = lo & ~15
    shift = lo - a0
    want_end = min(lo + GR_SEG + GR_STAGE_OVER, end)
    n_stage = want_end - a0
    at = shift + (o - lo)
    bs = _u32(buf, o)[0]
    return at + 4 + bs <= n_stage, shift, o + 4 + bs - want_end


def pack_path(buf, start, end):
    """for every record of the chain: (offset, 'stage' or 'mem', shift of its segment, record end minus want_end)"""
    out = []
    for o in chain(buf, start, end)[0]:
        st, shift, over = staged(buf, o, start, end)
        out.append((o, "stage" if st else "mem", shift, over))
    return out


def _aux_skip(buf, p, end):
    if p >= end:
        return -1
    t = buf[p]
    if t in b"AcC":
        return 2
    if t in b"sS":
        return 3
    if t in b"iIf":
        return 5
    if t == ord("d"):
        return 9
    if t in b"ZH":
        q = buf.find(b"\0", p + 1, end)
        return q - p + 1 if q >= 0 else -1
    if t == ord("B"):
        if end - p < 6:
            return -1
        esz = {99: 1, 67: 1, 115: 2, 83: 2, 105: 4, 73: 4, 102: 4}.get(buf[p + 1])
        if esz is None:
            return -1
        tot = 6 + _u32(buf, p + 2)[0] * esz
        return tot if tot <= end - p else -1
    return -1


def tag_values(buf, o, bs=None):
    """the raw values (type byte on) of the first CB, xf, GX and UB tag of the record at o, None where absent; bs: the
    block_size the parser believes (the record's own unless a mistake is being modelled)"""
    bs = _u32(buf, o)[0] if bs is None else bs
    rec = o + 4
    l_seq = _u32(buf, rec + 16)[0]
    fixed = min(32 + buf[rec + 8] + 4 * _u16(buf, rec + 12)[0] + (l_seq + 1) // 2 + l_seq, bs)
    aux, end = rec + fixed, rec + bs
    found = {}
    while end - aux >= 3:
        sz = _aux_skip(buf, aux + 2, end)
        if sz < 0:
            break
        found.setdefault(bytes(buf[aux:aux + 2]), bytes(buf[aux + 2:aux + 2 + sz]))
        aux += 2 + sz
    return tuple(found.get(t) for t in (b"CB", b"xf", b"GX", b"UB"))


WRONG = ("stitch compares only exits", "bases restart at segment 1024", "hop ignores end", "pack reads block_size from 32 KB",
         "repair stops after one segment")


def device(buf, start, end, n_ref, wrong=None):
    """what fastf_gpurec_parse returns for the window, kernel by kernel: dict(status, n, handover, offsets (SoA index -> record
    offset), repairs, windows, tags (SoA index -> tag_values))"""
    assert wrong is None or wrong in WRONG
    if end - start < 36:
        return dict(status=0, n=0, handover=start, offsets=[], repairs=0, windows=0, tags=[])
    segs, offs = hop(buf, start, end, n_ref, valid_end=len(buf) if wrong == WRONG[2] else None)
    exits = [t[1] for t in true_segments(buf, start, end)] if wrong == WRONG[0] else None
    n_seg, repairs = len(segs), 0
    if any(_bad(segs, i, exits) for i in range(1, n_seg)):
        repairs, segs, offs = repair(segs, buf, start, end, offs, one_only=wrong == WRONG[4], exits=exits)
    status = int(any(_bad(segs, i, exits) for i in range(1, n_seg)))
    if status:
        return dict(status=1, n=0, handover=start, offsets=[], repairs=repairs, windows=1, tags=[])
    base, carry = [], 0
    for s0 in range(0, n_seg, 1024):
        if wrong == WRONG[1]:
            carry = 0
        for s in range(s0, min(s0 + 1024, n_seg)):
            base.append(carry)
            carry += segs[s][2]
    n = carry
    soa = {}
    for s in range(n_seg):
        for k, o in enumerate(offs[s]):
            soa[base[s] + k] = o
    offsets = [soa.get(i) for i in range(n)]
    tags = []
    for o in offsets:
        if o is None:
            tags.append(None)
            continue
        bs = None
        if wrong == WRONG[3]:                                  # (bytes of the field behind the segment's own 32 KB read as zero)
            hi = start + ((o - start) // GR_SEG + 1) * GR_SEG
            bs = _u32(bytes(buf[o:min(o + 4, hi)]).ljust(4, b"\0"), 0)[0]
        tags.append(tag_values(buf, o, bs))
    return dict(status=0, n=n, handover=segs[-1][1], offsets=offsets, repairs=repairs, windows=1, tags=tags)


# ---------------------------------------------------------------- record and stream builders
def _bases(rng, n, alphabet=b"ACGT"):
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)])


def std_tags(rng):
    xf = (25, 25, 17, 0)[int(rng.integers(0, 4))]
    return (aux_Z(b"CB", _bases(rng, 16) + b"-1") + aux_int(b"xf", xf) + aux_Z(b"GX", b"ENSG%011d" % int(rng.integers(1, 5000))) +
            aux_Z(b"UB", _bases(rng, int(rng.integers(10, 13)))))


def b_array(payload):
    return b"ZBBC" + struct.pack("<I", len(payload)) + payload


def sized(total, name, tags, payload=None, tags_first=False, **shape):
    """a record of exactly `total` bytes (block_size field included): a `B` array in front of the tags (behind them with
    tags_first) makes up the size; payload: its first bytes, the rest zero"""
    bare = len(bam_record(name, tags, **shape))
    n = total - bare - 8
    assert n >= 0 and (payload is None or len(payload) <= n), (total, bare)
    arr = b_array((payload or b"").ljust(n, b"\0"))
    r = bam_record(name, tags + arr if tags_first else arr + tags, **shape)
    assert len(r) == total
    return r


def minimal(bs=32):
    """36 bytes: block_size 32, l_read_name 0, no aux; bs=31 gives the structurally invalid 35-byte form"""
    r = bytearray(bam_record(b"", b""))
    assert len(r) == 37
    del r[36:]
    r[12] = 0
    r[0:4] = struct.pack("<I", bs)
    return bytes(r[:4 + bs])


class Stream:
    """records appended one after the other; offsets are relative to the window's start"""

    def __init__(self, seed, pool=64):
        self.rng = np.random.default_rng(seed)
        self.b = bytearray()
        self.marks = {}
        self.pool = []
        for i in range(pool):
            total = int(self.rng.integers(150, 601))
            seq = int(self.rng.integers(0, 10))
            self.pool.append(sized(total, b"r%d" % i, std_tags(self.rng), seq_len=seq, n_cigar=i % 3 if seq else 0, ref_id=i % 3 - 1,
                                   pos=int(self.rng.integers(0, 1000))))

    @property
    def pos(self):
        return len(self.b)

    def add(self, rec, mark=None):
        if mark is not None:
            self.marks[mark] = len(self.b)
        self.b += rec
        return len(self.b) - len(rec)

    def mixed(self, n=1, mark=None):
        for _ in range(n):
            at = self.add(self.pool[int(self.rng.integers(0, len(self.pool)))], mark)
        return at

    def fill_to(self, target):
        """mixed records up to exactly `target`"""
        assert target - self.pos > 100 or target == self.pos, (target, self.pos)
        while target - self.pos > 700:
            self.mixed()
        if target > self.pos:
            self.add(sized(target - self.pos, b"f", aux_Z(b"CB", _bases(self.rng, 16) + b"-1") + aux_int(b"xf", 25)))
        assert self.pos == target

    def case(self, start, end_rel=None):
        return bytes(self.b), start, N_REF, start + (len(self.b) if end_rel is None else end_rel)


DECOY = bam_record(b"decoy", aux_Z(b"CB", b"AAAAAAAAAAAAAAAA-1") + aux_int(b"xf", 25) + aux_Z(b"GX", b"ENSG00000000001") +
                   aux_Z(b"UB", b"ACGTACGTAC"), seq_len=20, n_cigar=1, ref_id=0, pos=5)


def decoy_runoff(rng):
    """a record whose `B` array holds five decoy records 300 bytes in, zeros behind them, then the real tags"""
    return bam_record(b"enc", b_array(bytes(300) + DECOY * 5 + bytes(200)) + std_tags(rng))


def decoy_merge(rng):
    """the real tags, then a `B` array that ends the record with four decoy records: their chain runs into the true one"""
    return bam_record(b"enc", std_tags(rng) + b_array(bytes(300) + DECOY * 4))


# ---------------------------------------------------------------- the tag zoo (J)
CB16 = b"ACGTTGCAACGTTGCA"


def zoo():
    """[(kind, aux bytes)], the odd tails last in their aux block by construction"""
    cb, xf, gx, ub = aux_Z(b"CB", CB16 + b"-1"), aux_int(b"xf", 25), aux_Z(b"GX", b"ENSG00000000123"), aux_Z(b"UB", b"ACGTACGTAC")
    z = [("CB of type H", aux_Z(b"CB", CB16 + b"-1", b"H") + xf + gx + ub),
         ("CB twice", aux_Z(b"CB", b"TTTTTTTTTTTTTTTT-1") + xf + aux_Z(b"CB", CB16 + b"-2") + gx + ub)]
    for t in (b"c", b"C", b"s", b"S", b"i", b"I"):
        z.append(("xf of type " + t.decode(), cb + aux_int(b"xf", 25, t) + gx + ub))
    z += [("xf as f", cb + b"xff" + struct.pack("<f", 25.0) + gx + ub), ("xf as A", cb + b"xfA\x19" + gx + ub),
          ("xf negative c", cb + aux_int(b"xf", -25, b"c") + gx + ub)]
    for v in (17, 25, 24):
        z.append(("xf %d" % v, cb + aux_int(b"xf", v) + gx + ub))
    z += [("Z without NUL", cb + xf + ub + b"GXZENSG00000000123"),
          ("B count past the end", cb + xf + gx + b"ZBBC" + struct.pack("<I", 1000) + bytes(10)),
          ("B count past the end, tags behind", cb + xf + b"ZBBs" + struct.pack("<I", 40) + gx + ub),
          ("two spare bytes", cb + xf + gx + ub + b"XY")]
    for n in (0, 1, 16, 17):
        z.append(("UMI of %d" % n, cb + xf + gx + aux_Z(b"UB", (b"GATTACAGATTACAGAT")[:n])))
    z.append(("UMI with N", cb + xf + gx + aux_Z(b"UB", b"ACGTNCGTAC")))
    for n in (24, 25):
        z.append(("barcode of %d" % n, aux_Z(b"CB", (CB16 * 2)[:n]) + xf + gx + ub))
    for sfx in (b"-0", b"-254", b"-255", b"-01"):
        z.append(("barcode " + sfx.decode(), aux_Z(b"CB", CB16 + sfx) + xf + gx + ub))
    z += [("barcode with N", aux_Z(b"CB", b"ACGTNGCAACGTTGCA-1") + xf + gx + ub),
          ("barcode of 17 with N", aux_Z(b"CB", b"ACGTNGCAACGTTGCAA") + xf + gx + ub),
          ("gene with 13 digits", cb + xf + aux_Z(b"GX", b"ENSG1234567890123") + ub),
          ("gene with 14 digits", cb + xf + aux_Z(b"GX", b"ENSG12345678901234") + ub),
          ("second prefix", cb + xf + aux_Z(b"GX", b"ENSMUSG00000000003") + ub),
          ("unknown prefix", cb + xf + aux_Z(b"GX", b"ENSX00000000003") + ub),
          ("CB without xf", cb + gx + ub),
          ("CB and xf without GX", cb + xf + ub),
          ("no CB", xf + gx + ub),
          ("GX as integer", cb + xf + aux_int(b"GX", 7, b"i") + ub)]
    return z


BARCODES = b"".join(b + b"\n" for b in (CB16 + b"-1", b"AAAAAAAAAAAAAAAA-1", b"TTTTTTTTTTTTTTTT-1"))
FEATURES = b"".join(b"%s\tn\tGene Expression\n" % g for g in (b"ENSG00000000123", b"ENSG00000000001", b"ENSMUSG00000000003"))


# ---------------------------------------------------------------- the cases
def case_A():
    n = 3 * GR_SEG // 36
    return minimal() * n, 7, N_REF, 7 + 36 * n


def _mixed_stream():
    s = Stream(11)
    s.fill_to(2 * GR_SEG + GR_SEG // 2)
    return bytes(s.b)


def case_B(start):
    b = _mixed_stream()
    return b, start, N_REF, start + len(b)


EDGE_BACK = (1, 3, 4, 35, 36)


def case_C():
    s = Stream(12)
    for k, d in enumerate(EDGE_BACK, 1):
        s.fill_to(k * GR_SEG - d)
        s.add(sized(500, b"e", std_tags(s.rng)), mark="edge-%d" % d)       # (block_size 496: its second byte counts)
    s.fill_to(6 * GR_SEG)                                      # a record that ends exactly at hi: the guess is lane 0 of the first step
    s.marks["at-hi"] = s.pos
    s.fill_to(7 * GR_SEG - 200)
    s.add(sized(263, b"x", std_tags(s.rng)))                   # ends at lo + 63: the last candidate of the first step
    s.marks["slot-63"] = s.pos
    s.fill_to(8 * GR_SEG - 200)
    s.add(sized(264, b"x", std_tags(s.rng)))                   # ends at lo + 64: the first candidate of the second step
    s.marks["slot-64"] = s.pos
    s.fill_to(8 * GR_SEG + 1500)
    c = s.case(3)
    return c, s.marks


STAGE_ENDS = (-1, 0, 1, 20480)


def case_D():
    """in segment k (k = 0..3) the last record ends at lo + GR_SEG + GR_STAGE_OVER + STAGE_ENDS[k]; the one of segment 1 begins in
    the last 36 bytes of its segment; tags last, behind the `B` array"""
    s = Stream(13)
    for k, d in enumerate(STAGE_ENDS):
        begin = (k + 1) * GR_SEG - (20 if k == 1 else 500)
        s.fill_to(begin)
        s.add(sized((k + 1) * GR_SEG + GR_STAGE_OVER + d - begin, b"stage", std_tags(s.rng)), mark="stage%+d" % d)
    s.fill_to(6 * GR_SEG)
    return s.case(9), s.marks


def case_D_short():
    """the window ends 2000 bytes behind segment 1: want_end == end for segments 1 AND 2, and the last record of segment 1 ends
    exactly at `end`"""
    s = Stream(14)
    s.fill_to(2 * GR_SEG - 300)
    s.add(sized(2300, b"stage", std_tags(s.rng)), mark="last")
    return s.case(5), s.marks


LONG = (40 << 10, 70 << 10, 140 << 10)


def case_E(random_fill):
    s = Stream(15)
    rng = np.random.default_rng(1500)
    fill = (lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()) if random_fill else (lambda n: None)
    for i, n in enumerate(LONG + (LONG[1],)):
        s.add(sized(n, b"long", std_tags(s.rng), payload=fill(n - 200)), mark="long%d" % i)
        if i < 3:
            s.mixed(40)
    return s.case(0 if random_fill else 12), s.marks


def case_F(variant):
    s = Stream(16 + len(variant))
    s.fill_to(2 * GR_SEG - 200)
    if variant == "runoff":
        s.add(decoy_runoff(s.rng))
    elif variant == "merge":
        s.add(decoy_merge(s.rng))
    else:
        s.add(decoy_runoff(s.rng))
        s.fill_to(3 * GR_SEG - 200)
        s.add(decoy_runoff(s.rng))
    s.fill_to(4 * GR_SEG + 3000)
    return s.case(16)


CUTS = (1, 3, 4, 35, 36, "bs+3")


def case_G_cut(c):
    s = Stream(20)
    s.fill_to(GR_SEG + 3000)
    at = s.mixed()
    c = _u32(s.b, at)[0] + 3 if c == "bs+3" else c
    return s.case(2, at + c)


def case_G_tiny(n):
    return minimal()[:n], 1, N_REF, 1 + n


def case_G_last(k):
    """the last segment begins inside a long record and holds k plausible records before `end`"""
    s = Stream(21)
    s.fill_to(GR_SEG - 300)
    s.add(sized(2000, b"cross", std_tags(s.rng)))
    s.mixed(k)
    return s.case(4)


def case_G_refused():
    """segment 1 begins inside a long record; then two plausible records, one valid but implausible (ref_id beyond n_ref), more"""
    s = Stream(22)
    s.fill_to(GR_SEG - 300)
    s.add(sized(2000, b"cross", std_tags(s.rng)))
    s.marks["pair"] = s.pos
    s.mixed(2)
    s.add(bam_record(b"odd", std_tags(s.rng), ref_id=7, pos=1), mark="odd")
    s.marks["after"] = s.pos
    s.fill_to(2 * GR_SEG + 1000)
    return s.case(4), s.marks


def case_G_invalid():
    s = Stream(23)
    s.fill_to(GR_SEG + 5000)
    s.add(minimal(31), mark="invalid")
    s.fill_to(3 * GR_SEG + 1000)
    return s.case(6), s.marks


def case_H(which):
    """full: the window that leaves good records in the buffer; cut: the same bytes, `end` ten bytes short of a record's end in
    the middle of segment 1; edge: `end` on a record boundary there"""
    s = Stream(24)
    s.fill_to(GR_SEG + 9000)
    at = s.mixed()
    edge = s.pos
    s.fill_to(2 * GR_SEG + 7000)
    return s.case(13, {"full": None, "cut": edge - 10, "edge": edge}[which])


def case_I():
    s = Stream(25, pool=256)
    s.fill_to(1020 * GR_SEG - 200)
    s.add(decoy_runoff(s.rng))
    s.fill_to(1030 * GR_SEG - 200)
    s.add(decoy_runoff(s.rng))
    s.mixed(30)
    assert s.pos > 1024 * GR_SEG + 1
    return s.case(5)


def case_J():
    """the zoo four times over (32 or more kinds, so every kind meets lanes of both waves of the 128-thread workgroup); then every
    kind once more in a 6 KB record that begins 1000 bytes before the end of a segment of its own: the memory path"""
    s = Stream(26)
    z = zoo()
    for rep in range(4):
        for i, (kind, aux) in enumerate(z):
            s.add(bam_record(b"z%d.%d" % (rep, i), aux, seq_len=(rep * 7 + i) % 30, n_cigar=1 if (rep * 7 + i) % 30 else 0, ref_id=i % 3 - 1,
                             pos=i), mark=(kind, rep))
    k = s.pos // GR_SEG + 1
    for i, (kind, aux) in enumerate(z):
        s.fill_to((k + i + 1) * GR_SEG - 1000)
        bare = len(bam_record(b"big%d" % i, aux))
        s.add(bam_record(b"big%d" % i, b_array(bytes(6144 - bare - 8)) + aux), mark=(kind, "big"))
    s.fill_to(s.pos + 300)
    return s.case(10), s.marks


@functools.lru_cache(maxsize=None)
def case(name):
    """(bytes, start, n_ref, end) by name"""
    kind, _, arg = name.partition(".")
    if kind == "A":
        return case_A()
    if kind == "B":
        return case_B(int(arg))
    if kind == "C":
        return case_C()[0]
    if kind == "D":
        return (case_D_short() if arg == "short" else case_D())[0]
    if kind == "E":
        return case_E(arg == "random")[0]
    if kind == "F":
        return case_F(arg)
    if kind == "G":
        if arg.startswith("cut"):
            return case_G_cut(arg[3:] if arg[3:] == "bs+3" else int(arg[3:]))
        if arg.startswith("w"):
            return case_G_tiny(int(arg[1:]))
        if arg.startswith("last"):
            return case_G_last(int(arg[4:]))
        return (case_G_refused() if arg == "refused" else case_G_invalid())[0]
    if kind == "H":
        return case_H(arg)
    if kind == "I":
        return case_I()
    if kind == "J":
        return case_J()[0]
    raise KeyError(name)


B_STARTS = (0, 1, 5, 15, 16, 31)
H_CASES = ("H.full", "H.cut", "H.edge")
SMALL_CASES = (("A",) + tuple("B.%d" % s for s in B_STARTS) + ("C", "D", "D.short", "E.zeros", "E.random", "F.runoff", "F.merge", "F.two") +
               tuple("G.cut%s" % c for c in CUTS) + ("G.w35", "G.w36", "G.last1", "G.last2", "G.refused", "G.invalid", "J"))
ALL_CASES = H_CASES + SMALL_CASES + ("I",)


@functools.lru_cache(maxsize=None)
def image(name):
    """the device's window buffer for the case: offsets as the kernels see them"""
    b, start, _, _ = case(name)
    return bytes(start) + b


@functools.lru_cache(maxsize=None)
def expect(name):
    """device() for the case under the true rules"""
    _, start, n_ref, end = case(name)
    return device(image(name), start, end, n_ref)


# ---------------------------------------------------------------- a BAM file around a record stream (for the host reader)
def bam_file(records, n_ref=N_REF, level=1):
    """BAM header with n_ref references, then `records`, in BGZF blocks of 0xff00 bytes, with the EOF block"""
    text = b"@HD\tVN:1.6\n"
    pay = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_ref)
    for i in range(n_ref):
        nm = b"chr%d\0" % (i + 1)
        pay += struct.pack("<i", len(nm)) + nm + struct.pack("<i", 100000)
    pay += records
    out = []
    for a in range(0, len(pay), 0xff00):
        chunk = pay[a:a + 0xff00]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        data = co.compress(chunk) + co.flush()
        out.append(struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, ord("B"), ord("C"), 2, len(data) + 25) + data +
                   struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk)))
    out.append(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    return b"".join(out)
