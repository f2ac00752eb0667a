"""tests/grwin_ref.py (the expectations of tests/test_gpu_record_windows.py) against what the project already trusts, without a GPU:
its chain and its guess against the device functions compiled for the host (build/libgr_host.so, as tests/test_gpu_records_host.py
builds it), its record count against the host reader on the same records wrapped in a BAM file — whose packed SoA is then the
independent expectation of the device test.  Every case asserts, from the reference, that it reaches what it was built for; and
five plausible mistakes, put in place of one rule each in the reference, change the expectation of at least one case: the set
can see them, and no broken kernel has to run anywhere to show it.

What the reference shows about status 1: after gr_repair_kernel no window can be left out of step.  The walk rewrites every
segment it finds out of step from where the chain before it ends, goes on until a segment's own first record is met, and the
scan resumes behind that segment; a chain that stops early (invalid or cut record) leaves every later segment as (o, o, 0), which
is in step too.  `device()` returns status 0 for every case here, valid, cut or invalid; the fallback stays as the guard it is."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib

import grwin_ref as W
from test_bam_reader import read_all
from test_gpu_records_host import gr, views  # noqa: F401  (gr: the fixture that builds and loads libgr_host.so)

SEG = W.GR_SEG


@functools.lru_cache(maxsize=None)
def lists():
    return F.Lists(W.BARCODES, W.FEATURES)


@functools.lru_cache(maxsize=None)
def _host_records(records):
    """the host reader over `records` in a BAM file: (cb, gx, umi, meta, no_xf, no_gx); read_all must agree"""
    L = _lib.lib()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "w.bam")
        with open(path, "wb") as fh:
            fh.write(W.bam_file(records))
        cap = 50_000
        h = L.fastf_bam_open(path.encode(), 0)
        assert h, L.fastf_last_error()
        outs = [[], [], [], []]
        try:
            while True:
                a = [np.empty(cap, np.uint64), np.empty(cap, np.uint64), np.empty(cap, np.uint32), np.empty(cap, np.uint32)]
                n = L.fastf_bam_read_batch(h, lists().cell_dict, lists().feat_dict, *[x.ctypes.data for x in a], cap)
                assert n >= 0, L.fastf_last_error()
                if n == 0:
                    break
                for o, x in zip(outs, a):
                    o.append(x[:n].copy())
            nr, nxf, ngx = C.c_uint64(), C.c_uint64(), C.c_uint64()
            L.fastf_bam_stats(h, C.byref(nr), C.byref(nxf), C.byref(ngx))
        finally:
            L.fastf_bam_close(h)
        dt = (np.uint64, np.uint64, np.uint32, np.uint32)
        soa = [np.concatenate(o) if o else np.zeros(0, t) for o, t in zip(outs, dt)]
        assert nr.value == len(soa[0])
        for x, y in zip(soa, read_all(path, lists(), cap=7001)):
            assert np.array_equal(x, y)
    return soa + [nxf.value, ngx.value]


def expectation(name):
    """what the device must return for the case: n, handover, repairs and windows from the reference; the SoA, no_xf and no_gx from
    the host reader over the records in front of the reference's handover"""
    e = dict(W.expect(name))
    b, start, _, _ = W.case(name)
    *soa, no_xf, no_gx = _host_records(b[:e["handover"] - start])
    e.update(soa=soa, no_xf=no_xf, no_gx=no_gx)
    return e


def parse_host(gr, name):
    b, start, n_ref, end = W.case(name)
    img = W.image(name)
    cap = (end - start) // 36 + 2
    a = [np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)]
    vc, vf = views(lists())
    nxf, ngx, hand = C.c_uint32(), C.c_uint32(), C.c_uint64()
    n = gr.gr_host_parse(img, start, end, C.byref(vc), C.byref(vf), *[x.ctypes.data for x in a], cap, C.byref(nxf), C.byref(ngx), C.byref(hand))
    return n, hand.value, [x[:n] for x in a], nxf.value, ngx.value


@pytest.mark.parametrize("name", W.ALL_CASES)
def test_chain_device_and_host_reader_agree(gr, name):  # noqa: F811
    b, start, n_ref, end = W.case(name)
    img = W.image(name)
    offs, hand = W.chain(img, start, end)
    # the device functions on the host, one lane
    n, h, soa, nxf, ngx = parse_host(gr, name)
    assert (n, h) == (len(offs), hand)
    # the reference's kernels: status 0 without the fallback, the chain's records in the chain's order, within the SoA's room
    e = W.expect(name)
    assert e["status"] == 0 and e["offsets"] == offs and (e["n"], e["handover"]) == (len(offs), hand)
    assert e["n"] <= (end - start) // 36 + 1
    assert e["windows"] == (1 if end - start >= 36 else 0)
    # the host reader over the valid prefix: exactly the chain's count, and the SoA both packers agree on
    x = expectation(name)
    assert len(x["soa"][0]) == len(offs)
    for g, w in zip(soa, x["soa"]):
        assert np.array_equal(g, w)
    assert (nxf, ngx) == (x["no_xf"], x["no_gx"])
    if name in ("J", "C", "I"):
        assert len({tuple(int(a[i]) for a in x["soa"]) for i in range(len(offs))}) > 30      # (not all zeros: a real comparison)


@pytest.mark.parametrize("name", W.ALL_CASES)
def test_guess_equals_the_host_build_in_every_segment(gr, name):  # noqa: F811
    b, start, n_ref, end = W.case(name)
    img = W.image(name)
    for s in range(W.n_segments(start, end)):
        lo, hi = W.seg_range(s, start, end)
        assert W.guess(img, lo, hi, end, n_ref) == gr.gr_host_guess(img, lo, hi, end, n_ref), (name, s)


# ---------------------------------------------------------------- each case reaches what it claims
def _segs(name):
    b, start, n_ref, end = W.case(name)
    return W.hop(W.image(name), start, end, n_ref), W.true_segments(W.image(name), start, end)


def test_A_densest_segment():
    (segs, offs), true = _segs("A")
    assert len(segs) == 3 and segs[0][2] == 911 == W.GR_SEG_RECS - 1
    assert segs[1][0] == W.NONE and segs[2][0] == W.NONE and W.expect("A")["repairs"] == 2
    x = expectation("A")
    assert x["n"] == 2730 and not any(a.any() for a in x["soa"])


def test_B_every_shift():
    shifts = set()
    for st in W.B_STARTS:
        name = "B.%d" % st
        b, start, _, end = W.case(name)
        assert start == st and W.n_segments(start, end) == 3
        p = W.pack_path(W.image(name), start, end)
        assert {q[2] for q in p} == {st & 15}
        shifts.add(st & 15)
        assert W.expect(name)["n"] == W.expect("B.0")["n"]
    assert shifts == {0, 1, 5, 15}


def test_C_segment_edges():
    (b, start, n_ref, end), marks = W.case_C()
    img = W.image("C")
    offs = set(W.chain(img, start, end)[0])
    (segs, _), true = _segs("C")
    for d in W.EDGE_BACK:
        o = start + marks["edge-%d" % d]
        s = (o - start) // SEG
        assert o in offs and o == start + (s + 1) * SEG - d
        assert (o < start + (s + 1) * SEG < o + 4) == (d in (1, 3))          # the block_size field across the edge
        assert segs[s + 1] == true[s + 1]
    assert start + marks["at-hi"] == start + 6 * SEG and segs[6][0] == start + 6 * SEG
    assert segs[7][0] == start + 7 * SEG + 63 == start + marks["slot-63"] and segs[8][0] == start + 8 * SEG + 64 == start + marks["slot-64"]
    assert segs == true and W.expect("C")["repairs"] == 0


def test_D_both_sides_of_the_staging_test():
    (b, start, n_ref, end), marks = W.case_D()
    path = {o: (how, over) for o, how, _, over in W.pack_path(W.image("D"), start, end)}
    assert {q[2] for q in W.pack_path(W.image("D"), start, end)} == {9}
    want = {-1: "stage", 0: "stage", 1: "mem", 20480: "mem"}
    for d, how in want.items():
        assert path[start + marks["stage%+d" % d]] == (how, d)
    o = start + marks["stage+0"]
    assert start + 2 * SEG - 36 <= o < start + 2 * SEG                        # begins in the last 36 bytes of its segment
    tags = [W.tag_values(W.image("D"), start + marks["stage%+d" % d]) for d in want]
    assert all(None not in t for t in tags)                                   # CB, xf, GX and UB, all behind the B array
    assert sum(how == "mem" for how, _ in path.values()) == 2
    (b, start, n_ref, end), marks = W.case_D_short()
    p = {o: (how, over) for o, how, _, over in W.pack_path(W.image("D.short"), start, end)}
    assert end < start + SEG + SEG + W.GR_STAGE_OVER and p[start + marks["last"]] == ("stage", 0)      # want_end == end, met exactly
    assert W.true_segments(W.image("D.short"), start, end)[2][2] == 0


@pytest.mark.parametrize("name", ["E.zeros", "E.random"])
def test_E_consecutive_empty_segments(name):
    (segs, _), true = _segs(name)
    b, start, _, end = W.case(name)
    empty = [t[2] == 0 for t in true]
    assert any(empty[i] and empty[i + 1] and empty[i + 2] for i in range(len(empty) - 2))
    assert sum(empty) >= 6 and W.expect(name)["repairs"] >= sum(empty)
    offs, hand = W.chain(W.image(name), start, end)
    size = lambda o: W.rec_end(W.image(name), o, end) - o  # noqa: E731
    assert size(offs[0]) == W.LONG[0] and size(offs[-1]) == W.LONG[1] and hand == end
    assert sorted(size(o) for o in offs if size(o) > 1000) == sorted(W.LONG + (W.LONG[1],))


@pytest.mark.parametrize("variant,repairs", [("runoff", 1), ("merge", 1), ("two", 2)])
def test_F_decoys(variant, repairs):
    name = "F." + variant
    (segs, offs), true = _segs(name)
    b, start, n_ref, end = W.case(name)
    img = W.image(name)
    wrong = [s for s in range(1, len(segs)) if segs[s][0] != true[s][0]]
    assert wrong == ([2, 3] if variant == "two" else [2])
    for s in wrong:
        assert img[segs[s][0] + 36:segs[s][0] + 42] == b"decoy\0" and len(offs[s]) >= 3     # the guess is a decoy, decoys were hopped
        assert (segs[s][1] == true[s][1]) == (variant == "merge")               # merge: the right exit behind a wrong first
    e = W.expect(name)
    assert e["repairs"] == repairs
    assert not any(img[o + 36:o + 42] == b"decoy\0" for o in e["offsets"])


def test_G_window_end():
    for c in W.CUTS:
        name = "G.cut%s" % c
        b, start, n_ref, end = W.case(name)
        offs, hand = W.chain(W.image(name), start, end)
        bs = W._u32(W.image(name), hand)[0]
        assert end - hand == (bs + 3 if c == "bs+3" else c) and W.rec_end(W.image(name), hand, len(W.image(name))) == start + len(b)
        assert W.expect(name)["repairs"] == 0 and W.expect(name)["n"] == len(offs) > 50
    assert W.expect("G.w35") == dict(status=0, n=0, handover=1, offsets=[], repairs=0, windows=0, tags=[])
    e = W.expect("G.w36")
    assert (e["n"], e["handover"], e["windows"]) == (1, 37, 1)
    # the accepted guess: fewer than three plausible records, at the window's end
    for k in (1, 2):
        name = "G.last%d" % k
        (segs, offs), true = _segs(name)
        assert len(segs) == 2 and segs[1] == true[1] and segs[1][2] == k and true[1][0] > W.case(name)[1] + SEG + 1000
        assert W.expect(name)["repairs"] == 0
    # the refused guess: the same pair in the middle of a window
    (b, start, n_ref, end), marks = W.case_G_refused()
    (segs, offs), true = _segs("G.refused")
    assert true[1][0] == start + marks["pair"] and segs[1][0] == start + marks["after"]
    assert W.rec_end(W.image("G.refused"), start + marks["odd"], end) and not W.rec_plausible(W.image("G.refused"), start + marks["odd"], end, n_ref)
    assert W.expect("G.refused")["repairs"] == 1
    # the invalid record: the handover is at it
    (b, start, n_ref, end), marks = W.case_G_invalid()
    e = W.expect("G.invalid")
    assert e["handover"] == start + marks["invalid"] and e["status"] == 0 and e["n"] > 50
    assert e["repairs"] == 2 and W._u32(W.image("G.invalid"), e["handover"])[0] == 31


def test_H_good_records_lie_behind_end():
    full = W.expect("H.full")
    for name in ("H.cut", "H.edge"):
        b, start, n_ref, end = W.case(name)
        e = W.expect(name)
        assert W.case("H.full")[0] == b and end < W.case("H.full")[3]
        assert e["offsets"] == full["offsets"][:e["n"]] and e["n"] < full["n"] - 50
        assert W.rec_end(W.image(name), e["handover"], len(W.image(name))) != 0           # a whole good record begins at the handover
        assert (e["handover"] == end) == (name == "H.edge")


def test_I_more_than_1024_segments():
    (segs, offs), true = _segs("I")
    assert len(segs) > 1024
    wrong = [s for s in range(1, len(segs)) if segs[s] != true[s]]
    assert wrong == [1020, 1030] and W.expect("I")["repairs"] == 2
    sizes = np.diff(W.expect("I")["offsets"][:5000])
    assert sizes.min() >= 150 and sizes.max() <= 700 and len(set(sizes.tolist())) > 100
    assert len({t[2] for t in true}) > 20                                       # bases differ per segment


def test_J_every_kind_on_both_waves_and_on_the_memory_path():
    (b, start, n_ref, end), marks = W.case_J()
    img = W.image("J")
    true = W.true_segments(img, start, end)
    offs = W.chain(img, start, end)[0]
    index = {}                                                                  # record offset -> its index within its segment
    i = 0
    for s, t in enumerate(true):
        for k in range(t[2]):
            index[offs[i]] = k
            i += 1
    path = {o: how for o, how, _, _ in W.pack_path(img, start, end)}
    kinds = [k for k, _ in W.zoo()]
    assert len(kinds) == len(set(kinds)) >= 32
    for kind in kinds:
        waves = {(index[start + marks[(kind, rep)]] % 128) // 64 for rep in range(4)}
        assert waves == {0, 1}, kind
        assert {path[start + marks[(kind, rep)]] for rep in range(4)} == {"stage"}
        assert path[start + marks[(kind, "big")]] == "mem", kind
    x = expectation("J")
    assert x["no_xf"] >= 5 and x["no_gx"] >= 5
    # what the zoo is for, from the reference's own tag walk
    tv = {kind: W.tag_values(img, start + marks[(kind, 0)]) for kind in kinds}
    assert tv["CB twice"][0] == b"ZTTTTTTTTTTTTTTTT-1\0" and tv["CB of type H"][0][:1] == b"H"
    assert tv["Z without NUL"][2] is None and tv["B count past the end"][3] is None and tv["two spare bytes"][3] is not None
    assert tv["CB without xf"][1] is None and tv["CB and xf without GX"][2] is None
    for kind in kinds:
        assert W.tag_values(img, start + marks[(kind, "big")]) == tv[kind], kind


# ---------------------------------------------------------------- mistakes the set can see
def _differs(name, wrong):
    b, start, n_ref, end = W.case(name)
    e, w = W.expect(name), W.device(W.image(name), start, end, n_ref, wrong=wrong)
    return any(e[k] != w[k] for k in ("status", "n", "handover", "offsets", "repairs", "tags"))


SEES = {
    "stitch compares only exits": ["F.merge"],
    "bases restart at segment 1024": ["I"],
    "hop ignores end": ["H.cut"] + ["G.cut%s" % c for c in W.CUTS],
    "pack reads block_size from 32 KB": ["C"],
    "repair stops after one segment": ["F.two", "E.zeros", "E.random", "A"],
}


@pytest.mark.parametrize("wrong", W.WRONG)
def test_a_wrong_rule_changes_an_expectation(wrong):
    assert sorted(SEES) == sorted(W.WRONG)
    for name in SEES[wrong]:
        assert _differs(name, wrong), (wrong, name)
    e = W.expect("C")
    assert e["tags"] == [W.tag_values(W.image("C"), o) for o in e["offsets"]]
    # and a case built for something else does not see it by accident of its own (the rules are exercised, not the builders)
    assert not _differs("B.0", wrong)
