"""The fixture set of tests/deflate_ref.py on the CPU: the hand-written streams against zlib and the host build of the lane
decoder (tools/gi2_host.cpp), a census of what the token lists hold once the resolver's placement is replayed over them, and
the restated resolver (deflate_ref.resolve_batched) with one rule broken at a time: every broken rule but the cautious one must
change the bytes of some fixture.  tests/test_gpu_inflate.py runs the same set through bgzf_resolve_kernel.  No GPU."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

import deflate_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20


@pytest.fixture(scope="module")
def gi2():
    so = os.path.join(ROOT, "build", "libgi2_host.so")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "fastf_amd", "csrc"), so])
    L = C.CDLL(so)
    L.gi2_host_inflate.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    L.gi2_host_tokens.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def host_inflate(L, comp, n):
    out = C.create_string_buffer(max(n, 1)); nt = C.c_uint32()
    rc = L.gi2_host_inflate(comp, len(comp), out, n, C.byref(nt))
    return rc, out.raw[:n]


def host_tokens(L, comp, n):
    """(code, the block with its literals in place and 0xA5 where the matches go, tokens as uint32)"""
    out = C.create_string_buffer(b"\xA5" * max(n, 1)); nt = C.c_uint32()
    cap = D.token_cap(n)
    tok = np.zeros(cap, np.uint32)
    rc = L.gi2_host_tokens(comp, len(comp), out, n, tok.ctypes.data, cap, C.byref(nt))
    return rc, out.raw[:n], tok[:nt.value].copy()


@pytest.fixture(scope="module")
def fixtures():
    t0 = time.perf_counter()
    fx = D.resolver_fixtures(np.random.default_rng(SEED))
    assert time.perf_counter() - t0 < 10
    return [(name, s, n, D.inflate_ref(s)) for name, s, n in fx]


@pytest.fixture(scope="module")
def decoded(gi2, fixtures):
    """name -> (literals, tokens, expected) from phase 1 of the host build"""
    out = {}
    for name, s, n, exp in fixtures:
        rc, lits, tok = host_tokens(gi2, s, n)
        assert rc == 0, name
        out[name] = (lits, tok, exp)
    return out


def test_writer_zlib_and_host_decoder_agree(gi2, fixtures):
    """(resolver_fixtures has compared zlib's output with expand(tokens) for every stream that is one token list)"""
    assert 40 <= len(fixtures) and len(D.device_order([f[:3] for f in fixtures])) <= 400
    for name, s, n, exp in fixtures:
        assert len(exp) == n <= 65536, name
        rc, out = host_inflate(gi2, s, n)
        assert rc == 0 and out == exp, name
    rng = np.random.default_rng(5)
    for i in range(30):                                                  # the writer itself, on token lists of no design
        t = D._random_tokens(rng, 200)
        lit = D.complete_lengths(286, list(rng.permutation(286))); dist = D.complete_lengths(30, list(rng.permutation(30)))
        for s in (D.fixed_block(t), D.dynamic_block(t, lit, dist)):
            assert D.inflate_ref(s) == D.expand(t)
    for name, s, n in D.declined_fixtures():
        assert D.zlib_declines(s, n), name
        assert host_inflate(gi2, s, n)[0] != 0, name


def census(decoded):
    c = dict(mode0=set(), mode1=set(), mode2=set(), three_modes_in_a_round=[], depth=0, depth_overlap=0, cross_batch=0, n_tok=set(),
             lit_field=set(), skips=set(), dist_field=set(), cap_ratio=0.0, skip_lanes=set(), src0=0, ends_block=0, skip_only_batch=0,
             two_deps_with_gap=0, fan=0)
    for name, (lits, tok, exp) in decoded.items():
        c["n_tok"].add(len(tok))
        if len(exp): c["cap_ratio"] = max(c["cap_ratio"], len(tok) / D.token_cap(len(exp)))
        last = None                                                       # the last match of the batches in front: [dst, dend)
        for b, (lit, ln, dist, dst, src) in enumerate(D.place(tok)):
            n_here = min(64, len(tok) - 64 * b)
            m = ln != 0
            skip = ~m; skip[n_here:] = False
            c["skip_lanes"] |= set(np.flatnonzero(skip).tolist()); c["skips"] |= set(lit[skip].tolist())
            if skip[:n_here].all(): c["skip_only_batch"] += 1
            c["lit_field"] |= set(lit[m].tolist()); c["dist_field"] |= set((dist[m] - 1).tolist())
            mode = np.where(dist >= ln, 0, np.where(dist < 4, 1, 2))
            for i in np.flatnonzero(m):
                key = (int(src[i]) & 3, int(dst[i]) & 3, int(ln[i]))
                c["mode%d" % mode[i]].add(key + (int(dist[i]),) if mode[i] else key)
            c["src0"] += int((src[m] == 0).sum()); c["ends_block"] += int((dst[m] + ln[m] == len(exp)).sum())
            if last: c["cross_batch"] += int(((src[m] < last[1]) & (src[m] + np.minimum(ln[m], dist[m]) > last[0])).sum())
            deps = D.batch_deps(ln, dist, dst, src)
            depth = np.zeros(64, int); d_ov = np.zeros(64, int)
            for i in np.flatnonzero(m):
                j = np.flatnonzero(deps[i])
                depth[i] = 1 + (depth[j].max() if len(j) else 0)
                if dist[i] < ln[i]: d_ov[i] = 1 + (d_ov[j].max() if len(j) else 0)
                if len(j) >= 2 and dst[j[-1]] > dst[j[0]] + ln[j[0]]: c["two_deps_with_gap"] += 1
            c["depth"] = max(c["depth"], int(depth.max())); c["depth_overlap"] = max(c["depth_overlap"], int(d_ov.max()))
            c["fan"] = max(c["fan"], int(deps[:, 0].sum()) if m[0] else 0)
            for lanes in D.rounds(ln, deps):
                if set(mode[lanes].tolist()) == {0, 1, 2}: c["three_modes_in_a_round"].append((name, b))
            if m.any(): i = np.flatnonzero(m)[-1]; last = (int(dst[i]), int(dst[i] + ln[i]))
    return c


def test_census_of_the_fixture_set(decoded, fixtures):
    """What the set holds, counted on the token lists phase 1 makes of it with the kernel's placement replayed (conditions on
    the INPUTS of the device tests).  Mode 1 (distance 1..3 < length) fixes (src - dst) & 3 by its distance, so its grid is
    distance x destination phase x length: the twelve phase pairs a distance below 4 can have."""
    c = census(decoded)
    for length in D.GRID_LENS:
        for sp in range(4):
            for dp in range(4): assert (sp, dp, length) in c["mode0"], (sp, dp, length)
    for dist in (1, 2, 3):
        for length in D.SHORT_LENS:
            for dp in range(4):
                if length > dist: assert ((dp - dist) & 3, dp, length, dist) in c["mode1"], (dist, dp, length)
    for dist in D.LONG_DISTS:
        for length in {dist + 1, min(2 * dist, 258), 258}:
            if length > dist: assert {dp for (_, dp, l, d) in c["mode2"] if (l, d) == (length, dist)} == {0, 1, 2, 3}, (dist, length)
    assert c["three_modes_in_a_round"]
    assert c["depth"] >= 64 and c["depth_overlap"] >= 64 and c["cross_batch"] >= 1 and c["fan"] == 63 and c["two_deps_with_gap"] >= 1
    assert {0, 1, 63, 64, 65, 128, 129} <= c["n_tok"] and max(c["n_tok"]) >= 200
    assert {0, 254, 255} <= c["lit_field"] and {256, 257, 511, 512, 65533, 65535, 60001} <= c["skips"]
    assert {0, 63} <= c["skip_lanes"] and c["skip_only_batch"] >= 1
    assert {0, 1, 2, 32505, 32506, 32766, 0x7FFF} <= c["dist_field"]
    assert 0.98 <= c["cap_ratio"] <= 1.0
    assert c["src0"] >= 4 and c["ends_block"] >= 4
    # the launch of the device tests: every fixture at the four values of uoff & 3, a first wave of one long and 63 tiny blocks
    order = D.device_order([f[:3] for f in fixtures])
    uoffs, _ = D.layout(order)
    assert 257 <= len(order) <= 400
    assert order[0][2] == 65536 and all(e[2] <= 3 for e in order[1:64])
    for name in decoded:
        assert {u & 3 for u, e in zip(uoffs, order) if e[0] == name} == {0, 1, 2, 3}, name


def test_each_wrong_rule_changes_some_fixture(decoded):
    """the restated schedule gives zlib's bytes on every fixture, and so does the cautious dependency range; each of the other
    five wrong rules is caught by at least one fixture"""
    for name, (lits, tok, exp) in decoded.items():
        assert D.resolve_batched(lits, tok) == exp, name
        assert D.resolve_batched(lits, tok, "deps_len") == exp, name
    small = sorted(decoded, key=lambda n: len(decoded[n][1]))
    for defect in D.DEFECTS:
        if defect == "deps_len": continue
        caught = [n for n in small if len(decoded[n][1]) <= 1000 and D.resolve_batched(decoded[n][0], decoded[n][1], defect) != decoded[n][2]]
        assert caught, "no fixture notices the defect %s" % defect
        print("%s: caught by %d fixtures, first %s" % (defect, len(caught), ", ".join(caught[:4])))
    # the fixtures built for a rule are among those that notice it
    bad = lambda n, d: D.resolve_batched(decoded[n][0], decoded[n][1], d) != decoded[n][2]
    assert bad("chain/64", "no_deps") and bad("chain/fan_out", "no_deps") and bad("chain/straddle", "no_deps")
    assert bad("short_overlap", "no_rotate3") and bad("short_overlap", "plain_overlap") and bad("long_overlap/dst1", "plain_overlap")
    assert bad("stepover/lane0", "lit8_skip") and bad("tokens/65", "batch_pos") and not bad("tokens/64", "batch_pos")
