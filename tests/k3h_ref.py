"""reduce_hashed_kernel<false> (K3h, the 32-bit window set) and giant_groups_kernel restated in plain Python and numpy (uint64,
exact), with hand-built key arrays that put every key on a chosen lane, unit, wave and window.

No tests here: tests/test_k3h_ref_host.py checks these helpers against sortreduce_ref.want_rows, takes a census of the fixtures
and runs the reference mutants; tests/test_gpu_k3h_windows.py uploads the fixtures as they are (no sort in front) and compares
the device's rows and error bit with expect().

A window is 2048 keys.  Wave w owns positions 256 w .. 256 w + 255, unit j of wave w positions 256 w + 64 j .. + 63."""
import itertools

import numpy as np

from sortreduce_ref import CS, FS, want_rows

U = np.uint64
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
TILE, WAVE, THREADS = 2048, 64, 512                      # K3H_TILE, WAVE, K3H_THREADS
TAB32, LO32 = 8192, 13                                   # K3H_TAB32, K3H_LO32
MAX_TRIES = 63                                           # probes of one key: the most a chain holds
GIANT_MAX, GIANT_PART, GIANT_LIST_CAP, GIANT_TAB = 1 << 16, 1536, 4096, 4096
GOLD64 = 0x9E3779B97F4A7C15


class Layout:
    """[cell][feature 9][nonnull 1][umi][len 2]: where the group, the cell and the NULL flag of a key are"""

    def __init__(self, feat_shift=FS, cell_shift=CS, nn_shift=None, feat_bits=9):
        self.fs, self.cs, self.feat_bits = feat_shift, cell_shift, feat_bits
        self.nn = feat_shift - 1 if nn_shift is None else nn_shift
        self.umi_bits = self.nn - 2

    def group(self, i):
        """group word number i, ascending in i: cell 1 + i // 500, feature 1 + i % 500 (listed ones for i < 500 000)"""
        return ((1 + i // 500) << self.cs) | ((1 + i % 500) << self.fs)

    def x_of(self, t, ln=3):
        """non-NULL key bits below the group for token t: the UMI is a bijection of t that spreads over every bit of hi"""
        return (1 << self.nn) | (((t * 0x9E3779B1 + 0x3039) & ((1 << self.umi_bits) - 1)) << 2) | ln


L12 = Layout(27, 36)                                     # 12 bases: the fixture engine of test_gpu_kernels.py
L10 = Layout(23, 32)                                     # 10 bases

# what a mutant of the reference changes (tests/test_k3h_ref_host.py)
RULES = dict(hi_mask=~0, rank_in_word=True, probe_in_word=True, max_tries=MAX_TRIES, clear_set=True, copy_across_head=False,
             single_at_lane63=False, stop_beyond=False, giant_max=GIANT_MAX, part_low_half=False)


def umul24(a, b):
    return ((a & 0xFFFFFF) * (b & 0xFFFFFF)) & M32


def slot32(x, r, rules=RULES):
    """(home slot, step, word of the first probe) of key bits x in the group of row rank r; the word of probe i adds i << 26"""
    x = int(x)
    hi = x >> LO32
    f = umul24(hi, 0x9E3779)
    slot = (x ^ (f >> 8) ^ umul24(r, 0x9E5)) & (TAB32 - 1)
    word = (hi & rules["hi_mask"] & M32) | ((r << 15) if rules["rank_in_word"] else 0) | (1 << 26)
    return slot, ((f >> 20) & 62) | 1, word


def k3_chunk_start(n, b, G):
    T = (n + TILE - 1) // TILE
    s = (T * b // G) * TILE
    return min(s, n)


def giant_partition(key, parts, rules=RULES):
    hh = (int(key) * GOLD64) & M64
    return (((hh & M32) if rules["part_low_half"] else (hh >> 32)) * parts) >> 32


# ---------------------------------------------------------------------------------------------------------------------
# chunks, windows, cuts
# ---------------------------------------------------------------------------------------------------------------------
def geometry(keys, max_n, lay=L12, rules=RULES, detail=False):
    """the windows of a launch sized for max_n keys as (chunk, base, cut, giant, len, parts); detail: also (how each window was
    cut: 'stop' / 'end' / 'last' / 'giant', the chunks without rows, lim of each window)"""
    keys = np.asarray(keys, np.uint64)
    n = len(keys)
    G = max((max_n + TILE - 1) // TILE, 1)
    assert n <= max_n and G <= 64                        # beyond 64 tiles the grid depends on the device's CU count
    grp = keys >> U(lay.fs)
    head = np.ones(n, dtype=bool)
    head[1:] = grp[1:] != grp[:-1]
    hpos = np.flatnonzero(head)
    wins, how, empty, lims = [], [], [], []
    for b in range(G):
        s, e = k3_chunk_start(n, b, G), k3_chunk_start(n, b + 1, G)
        cursor = s
        if b > 0 and s < e:
            i = np.searchsorted(hpos, s)                 # the first head at or after the nominal start
            cursor = int(hpos[i]) if i < len(hpos) and hpos[i] < e else e
        if cursor >= e:
            empty.append(b)
            continue
        done = False
        while not done:
            base = cursor
            W = min(n - base, TILE)
            lim = min(e - base, TILE) if e > base else 0
            h = np.flatnonzero(head[base:base + W])
            if W:
                assert h[0] == 0                         # a window starts at a head
            stop = h[h > lim] if rules["stop_beyond"] else h[h >= lim]
            lims.append(lim)
            if lim < TILE and len(stop):
                wins.append((b, base, int(stop[0]), False, 0, 0)); how.append("stop"); done = True
                cursor = base + int(stop[0])
            elif base + W == n:
                wins.append((b, base, W, False, 0, 0)); how.append("end"); done = True
            elif len(h) > 1:
                wins.append((b, base, int(h[-1]), False, 0, 0)); how.append("last")
                cursor = base + int(h[-1])
            else:
                i = np.searchsorted(hpos, base + W)
                nxt = int(hpos[i]) if i < len(hpos) else n
                ln = nxt - base
                wins.append((b, base, W, True, ln, (ln + GIANT_PART - 1) // GIANT_PART)); how.append("giant")
                cursor = nxt
                done = cursor >= e or cursor >= n
    return (wins, how, empty, lims) if detail else wins


class Lanes:
    """what every position of one window is to the kernel: head, copy of the neighbour in front, single head, row rank, probing"""

    def __init__(self, keys, base, cut, lay, rules=RULES):
        n = len(keys)
        W = min(n - base, TILE)
        k = np.asarray(keys[base:base + W], np.uint64)
        pos = np.arange(W)
        prev = np.concatenate([[U(0)], k[:-1]])          # position 0: the carry in front of wave 0 is zero
        xm = U((1 << lay.fs) - 1)
        head = (pos == 0) | ((k >> U(lay.fs)) != (prev >> U(lay.fs)))
        same = ~head & (k == prev)
        if rules["copy_across_head"]:
            same = (pos > 0) & ((k & xm) == (prev & xm))
        is_head = head & (pos < cut)
        nxt = np.concatenate([is_head[1:], [False]])
        single = is_head & nxt & (pos % WAVE != WAVE - 1)
        if rules["single_at_lane63"]:
            single = is_head & (nxt | (pos % WAVE == WAVE - 1))
        nonnull = ((k >> U(lay.nn)) & U(1)) == 1
        self.k, self.x, self.pos = k, (k & xm), pos
        self.head, self.same, self.single, self.is_head = head, same, single, is_head
        self.r = np.cumsum(is_head) - 1
        self.dist = (pos < cut) & nonnull & ~same
        self.probe = self.dist & ~single
        self.n_rows = int(is_head.sum())


def probe_all(items, rules=RULES, tab=None):
    """the set of one window, keys (r, x) inserted in the given order: (indices found as seen before, any key not placed)"""
    tab = {} if tab is None else tab
    seen, overflow = [], False
    for i, (r, x) in enumerate(items):
        s, step, w = slot32(x, r, rules)
        for t in range(rules["max_tries"]):
            got = tab.get(s, 0)
            if got == 0:
                tab[s] = w
                break
            if got == w:
                seen.append(i)
                break
            s = (s + step) & (TAB32 - 1)
            if rules["probe_in_word"]:
                w += 1 << 26
        else:
            overflow = True
    return seen, overflow


def chain_walk(x, r):
    s, step, _ = slot32(x, r)
    return [(s + i * step) & (TAB32 - 1) for i in range(MAX_TRIES)]


def order_independent(items):
    """whether the outcome of a window cannot depend on the order its keys reach the set.  Keys that share home slot and step
    are a chain; apart from chain members no two distinct (r, x) share a home slot, and no such home slot lies on the 63-slot
    walk of a chain, nor do the walks of two chains meet.  A window that probes at most six keys may instead be shown
    order-independent by running every order."""
    distinct = list(dict.fromkeys(items))
    by_home = {}
    for r, x in distinct:
        s, step, _ = slot32(x, r)
        by_home.setdefault(s, []).append((r, x, step))
    ok = True
    walks = {}
    for s, members in by_home.items():
        if len(members) > 1:
            if len({m[2] for m in members}) != 1:
                ok = False
            walks[s] = set(chain_walk(members[0][1], members[0][0]))
    for s, w in walks.items():
        if any(t != s and t in w for t in by_home):
            ok = False
        if any(s2 != s and (w & w2) for s2, w2 in walks.items()):
            ok = False
    if ok or len(items) > 6:
        return ok
    outs = set()
    for p in itertools.permutations(range(len(items))):
        seen, ov = probe_all([items[i] for i in p])
        outs.add((tuple(sorted(items[p[i]] for i in seen)), ov))
    return len(outs) == 1


def expect(keys, max_n, lay=L12, rules=RULES):
    """((feature, cell, count) rows in order of appearance, flagged, [order_independent per window]).  The count of a group the
    kernels could not hold (which raises the flag) is its exact one: what the full sort and reduce then gives."""
    keys = np.asarray(keys, np.uint64)
    wins = geometry(keys, max_n, lay, rules)
    fmask = (1 << lay.feat_bits) - 1
    rows, indep, flagged, items_total = [], [], False, 0
    tab, tab_chunk = {}, -1
    for b, base, cut, giant, ln, parts in wins:
        if b != tab_chunk or rules["clear_set"]:
            tab, tab_chunk = {}, b
        if giant:
            g = keys[base:base + ln]
            nn = np.unique(g[((g >> U(lay.nn)) & U(1)) == 1])
            count = len(nn)
            if ln > rules["giant_max"]:
                flagged = True
            else:
                items_total += parts
                per = np.bincount([giant_partition(k, parts, rules) for k in nn.tolist()], minlength=parts) if len(nn) else np.zeros(1, int)
                if per.max() > GIANT_TAB:
                    flagged = True
            k0 = int(keys[base])
            rows.append(((k0 >> lay.fs) & fmask, k0 >> lay.cs, count))
            indep.append(True)
            continue
        L = Lanes(keys, base, cut, lay, rules)
        pi = np.flatnonzero(L.probe)
        items = [(int(L.r[i]), int(L.x[i])) for i in pi]
        seen, overflow = probe_all(items, rules, tab)
        indep.append(order_independent(items))
        cnt = np.bincount(L.r[L.dist], minlength=L.n_rows) - np.bincount(L.r[pi[seen]], minlength=L.n_rows)
        if overflow:                                     # the flag is up: the rows come from the full sort
            flagged = True
            cnt = np.array([len(set(L.x[(L.r == r) & (L.pos < cut) & (((L.k >> U(lay.nn)) & U(1)) == 1)].tolist())) for r in range(L.n_rows)])
        for r, i in enumerate(np.flatnonzero(L.is_head)):
            k0 = int(L.k[i])
            rows.append(((k0 >> lay.fs) & fmask, k0 >> lay.cs, int(cnt[r])))
    if items_total > GIANT_LIST_CAP:
        flagged = True
    return rows, flagged, indep


def rows_arrays(rows):
    a = np.array(rows, dtype=np.int64).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2]


# ---------------------------------------------------------------------------------------------------------------------
# chains and one-partition keys
# ---------------------------------------------------------------------------------------------------------------------
def step_classes(lay=L12):
    """non-NULL values of hi by step class: 32 classes of 253 to 258 values in the 12-base layout, 13 to 19 in the 10-base one"""
    out = {}
    top = 1 << (lay.nn - LO32)
    for hi in range(top, 2 * top):
        out.setdefault(((umul24(hi, 0x9E3779) >> 20) & 62) | 1, []).append(hi)
    return out


def chain32(m, target_slot, lay=L12, step=None):
    """m distinct non-NULL x that share home slot and step: one x per hi of one step class, lo = target ^ (f >> 8).  The row rank
    enters the slot as an XOR common to all members: a chain for one rank is a chain for every rank (its home: target ^ g(r))"""
    classes = step_classes(lay)
    step = max(classes, key=lambda s: len(classes[s])) if step is None else step
    his = classes[step]
    assert m <= len(his), (m, len(his))
    return np.array([(hi << LO32) | ((target_slot ^ (umul24(hi, 0x9E3779) >> 8)) & (TAB32 - 1)) for hi in his[:m]], dtype=np.uint64)


def hi_alias_pair(target_slot, lay=L12):
    """two x of one step class and one home slot whose hi agree in their low 8 bits ([] where the layout has none)"""
    for step, his in sorted(step_classes(lay).items()):
        by = {}
        for hi in his:
            by.setdefault(hi & 0xFF, []).append(hi)
        for pair in by.values():
            if len(pair) >= 2:
                return [(hi << LO32) | ((target_slot ^ (umul24(hi, 0x9E3779) >> 8)) & (TAB32 - 1)) for hi in pair[:2]]
    return []


def one_partition_keys(group, parts, part, m, lay=L12):
    """m distinct non-NULL keys of group word `group` that fall into hash partition `part` of `parts`: UMIs 0, 1, 2, .. scanned"""
    out, umi = [], 0
    while len(out) < m:
        k = group | (1 << lay.nn) | (umi << 2) | 3
        if giant_partition(k, parts) == part:
            out.append(k)
        umi += 1
        assert umi < 1 << lay.umi_bits
    return np.array(out, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------------
class Fixture:
    def __init__(self, family, keys, max_n, lay):
        self.family, self.keys, self.max_n, self.lay = family, np.asarray(keys, np.uint64), int(max_n), lay


def settle(keys, max_n, lay, pinned=()):
    """re-picks the low 13 bits of keys that are not pinned so that, window by window, no two distinct (row rank, x) share a home
    slot and none sits on the walk of a pinned chain; equal keys stay equal, distinct ones distinct, hi is kept"""
    keys = np.array(keys, dtype=np.uint64)
    pinned = set(int(k) for k in pinned)
    for b, base, cut, giant, ln, parts in geometry(keys, max_n, lay):
        if giant:
            continue
        L = Lanes(keys, base, cut, lay)
        items = list(dict.fromkeys((int(L.r[i]), int(L.k[i])) for i in np.flatnonzero(L.probe)))
        xm = (1 << lay.fs) - 1
        used, homes = set(), {}
        for r, k in items:
            if k in pinned:
                homes.setdefault(slot32(k & xm, r)[0], []).append((r, k))
        for s, mem in homes.items():
            used.add(s)
            if len(mem) > 1:
                used.update(chain_walk(mem[0][1] & xm, mem[0][0]))
        free = 0
        for r, k in items:
            if k in pinned:
                continue
            x = k & xm
            s = slot32(x, r)[0]
            if s in used:
                while free in used:
                    free += 1
                hi = x >> LO32
                x = (hi << LO32) | ((free ^ (umul24(hi, 0x9E3779) >> 8) ^ umul24(r, 0x9E5)) & (TAB32 - 1))
                s = free
                new = (k & ~xm) | x
                sel = keys[base:base + cut] == U(k)
                keys[base:base + cut][sel] = U(new)
            used.add(s)
    return keys


def from_heads(lay, head, tok, first_group=0, xs=None):
    """keys from per-position head flags and tokens (token < 0: a NULL key; xs: explicit key bits per position, 0 = none)"""
    head = np.asarray(head, bool).copy()
    head[0] = True
    g = np.cumsum(head) - 1 + first_group
    out = np.empty(len(head), np.uint64)
    for i in range(len(head)):
        x = 0 if tok[i] < 0 else lay.x_of(int(tok[i]))
        if xs is not None and xs[i]:
            x = int(xs[i])
        out[i] = lay.group(int(g[i])) | x
    return out


def from_sizes(lay, sizes, first_group=0, dup=3, null_every=11, tok0=0):
    """groups of the given sizes; tokens run on, every dup-th key of a group repeats an earlier token of it, every
    null_every-th is NULL"""
    head, tok = [], []
    t = tok0
    for s in sizes:
        mine = []
        for j in range(s):
            head.append(j == 0)
            if null_every and (len(head) % null_every) == 0:
                tok.append(-1)
            elif dup and mine and j % dup == 0:
                tok.append(mine[(j * 7) % len(mine)])
            else:
                mine.append(t); tok.append(t); t += 1
    return from_heads(lay, np.array(head), np.array(tok), first_group)


def _filler(n, period=8, offset=4):
    """head flags and tokens of n positions: groups of `period` keys whose edges sit at offset mod period, distinct tokens"""
    pos = np.arange(n)
    return (pos % period == offset) | (pos == 0), pos.copy()


PAIR = [300] + [40] * 30 + [700]                         # 2200 keys: a window of 31 groups, cut at 1500, then a window of one


def window_pairs(lay, k, first_group=0, lead=None):
    """k times PAIR.  With chunks of one tile (every launch of at most 64 tiles) a workgroup runs at most two windows that use the
    set: one cut at its last head, then the group left open, alone, at row rank 0.  Here that group repeats the key bits of the
    first window's rank-0 group under another cell: a set or a count left behind by the first window turns it wrong.
    lead: key bits for the first 300-key group (else tokens)"""
    head = np.zeros(2200 * k, bool)
    tok = np.zeros(2200 * k, np.int64)
    xs = np.zeros(2200 * k, np.uint64)
    for i in range(k):
        o = 2200 * i
        head[o + np.concatenate([[0], np.cumsum(PAIR)[:-1]])] = True
        a = np.arange(300) % 211                         # 211 distinct tokens, 89 of them twice
        a[::13] = -1
        tok[o:o + 300] = a
        tok[o + 300:o + 1500] = 1000 + np.arange(1200) % 17 + 17 * (np.arange(1200) // 40)
        tok[o + 1500:o + 2200] = np.concatenate([a, a, a[:100]])
        if lead is not None:
            xs[o:o + len(lead)] = lead
    return from_heads(lay, head, tok, first_group, xs=xs if lead is not None else None)


def _repeat_lead(keys, lay, k, offset=0):
    """after settle(): the 700-key group of every pair takes the (settled) key bits of its pair's 300-key group"""
    xm = U((1 << lay.fs) - 1)
    for i in range(k):
        o = offset + 2200 * i
        a = keys[o:o + 300] & xm
        b = keys[o + 1500:o + 2200]
        keys[o + 1500:o + 2200] = (b & ~xm) | np.concatenate([a, a, a[:100]])
    return keys


def _fixtures(lay):
    F = {}
    G = lay.group

    def add(name, family, keys, max_n=None, pinned=(), settle_it=True):
        keys = np.asarray(keys, np.uint64)
        max_n = len(keys) if max_n is None else max_n
        F[name] = Fixture(family, settle(keys, max_n, lay, pinned) if settle_it else keys, max_n, lay)

    # ---- neighbour copies -----------------------------------------------------------------------------------------
    for name, key0 in (("copies_at_lane0", False), ("copies_key0_first", True)):
        head, tok = _filler(TILE)
        for p in [1, 64, 128, 192, 2047] + [256 * w for w in range(1, 8)]:
            tok[p] = tok[p - 1]                          # a pair whose second member sits at p
        tok[830:834] = tok[830]                          # a run of four across the edge of unit 13
        head[310:451] = False; tok[310:451] = tok[310]   # one key 141 times across units 4 to 7
        head[600:701] = False; tok[600:701] = -1         # a run of NULL keys across units 9 and 10
        keys = from_heads(lay, head, tok)
        if key0:
            head[1] = True
            keys = from_heads(lay, head, tok, first_group=-1)
            keys[0] = 0                                  # cell 0, feature 0, NULL: the value of the carry in front of wave 0
            keys[1:4] = U(G(0)) | U(lay.x_of(1))         # ... then a group of three copies: a pair whose second member sits at 2
        add(name, "neighbour copies", keys)

    # ---- single heads ---------------------------------------------------------------------------------------------
    n = TILE
    tok = np.arange(n); tok[::7] = -1
    add("singles_2048", "single heads", from_heads(lay, np.ones(n, bool), tok))
    head, tok = _filler(TILE)
    for u in range(1, 32):
        head[64 * u - 2:64 * u + 2] = True               # singles at lanes 62, 63 and 0 around every unit edge
    tok[64 * 5 - 1] = -1; tok[64 * 9] = -1
    add("singles_unit_edges", "single heads", from_heads(lay, head, tok))
    head, tok = _filler(TILE)
    xs = np.zeros(TILE, np.uint64)
    for i, p in enumerate([10, 64 * 3 + 61, 64 * 7 + 62, 64 * 11 + 63, 64 * 16, 64 * 20 + 1, 256 * 5 + 60, 256 * 6 + 62]):
        head[p:p + 4] = [True, True, False, True]        # a single, then a group of two equal keys: all three the same x
        xs[p:p + 3] = lay.x_of(5000 + i)
        tok[p + 3] = 100_000 + i
    keys = from_heads(lay, head, tok, xs=xs)
    add("single_then_equal_pair", "single heads", keys, pinned=keys[xs != 0])

    # ---- counts across units --------------------------------------------------------------------------------------
    head, tok = _filler(TILE)
    head[100:801] = False; head[100] = True
    tok[100:256] = np.arange(156); tok[256:412] = np.arange(156); tok[412:768] = 156 + np.arange(356); tok[768:801] = np.arange(33)
    head[801:960] = False
    for p in (801, 816, 820, 832, 959):                  # NULL groups between counted ones; unit 13: its only head at lane 0,
        head[p] = True                                   # unit 14: its only head at lane 63
    tok[801:816] = -1; tok[820:832] = -1
    tok[832:959] = 600 + np.arange(127) % 40
    head[960:1100] = False; tok[959:1100] = 700 + np.arange(141) % 50
    add("counts_across_units", "counts across units", from_heads(lay, head, tok))
    add("one_then_2046", "counts across units", from_sizes(lay, [1, 2046, 5, 1, 30, 9]))

    # ---- set words ------------------------------------------------------------------------------------------------
    def set_words(twice, t):
        x0 = lay.x_of(0x2A5A5 + t)
        variants = [x0, x0 ^ (1 << 12), x0 ^ (1 << 13), x0 ^ (1 << (lay.nn - 1)), x0 ^ 1, x0 ^ 2, x0 ^ 0x555, x0 ^ (0x15 << 13)]
        alias = hi_alias_pair(4000 + 97 * t, lay)        # same home, same step, hi equal in its low 8 bits (12 bases only)
        x1, x2, x3 = lay.x_of(777_001 + 3 * t), lay.x_of(777_002 + 3 * t), lay.x_of(777_003 + 3 * t)
        groups = [variants + alias + [x1, x2], [x1, x2], [x2, lay.x_of(9)]]
        groups += [[x3, lay.x_of(50 + i)] for i in range(64)]
        # the same hi under two row ranks with one home slot: lo differs by g(r1) ^ g(r2)
        ra, rb = len(groups), len(groups) + 1
        xa = lay.x_of(888_001 + t)
        xb = (xa & ~(TAB32 - 1)) | ((xa ^ umul24(ra, 0x9E5) ^ umul24(rb, 0x9E5)) & (TAB32 - 1))
        groups += [[xa, lay.x_of(1)], [xb, lay.x_of(2)]]
        pinned, parts = [], []
        hold = set(variants + alias + [x1, x2, x3, xa, xb])
        for gi, xs_ in enumerate(groups):
            ks = [G(gi) | x for x in xs_]
            pinned += [G(gi) | x for x in xs_ if x in hold]
            if twice and gi < 3:                         # every key twice, the copies 300 keys on: another wave
                ks = ks + [G(gi) | lay.x_of(10_000 + 400 * gi + j) for j in range(300)] + ks
            elif twice:
                ks = ks + [G(gi) | lay.x_of(3)] + ks     # twice, not adjacent
            parts.append(np.array(ks, dtype=np.uint64))
        keys = np.concatenate(parts)
        return settle(keys, len(keys), lay, pinned)

    def first_clean(build):
        """the first of a family of candidates whose windows all satisfy the order-independence condition"""
        for t in range(200):
            keys = build(t)
            if all(expect(keys, len(keys), lay)[2]):
                return keys
        raise AssertionError("no candidate is order-independent")
    add("set_words", "set words", first_clean(lambda t: set_words(False, t)), settle_it=False)
    add("set_words_twice", "set words", first_clean(lambda t: set_words(True, t)), settle_it=False)

    # ---- twin windows ---------------------------------------------------------------------------------------------
    def add_pairs(name, front, k, first, lead=None, pinned=()):
        keys = settle(np.concatenate([front, window_pairs(lay, k, first, lead)]), len(front) + 2200 * k, lay, pinned)
        keys = _repeat_lead(keys, lay, k, len(front))
        if lead is not None and len(lead) > MAX_TRIES:   # the second window holds what a chain can hold: it is exact if the set was cleared
            tail = keys[len(front) + 1500:]
            xm = U((1 << lay.fs) - 1)
            tail[np.isin(tail & xm, lead[MAX_TRIES:])] = (tail[0] & ~xm) | lead[0]
        F[name] = Fixture("twin windows", keys, len(keys), lay)
    add_pairs("twin2", np.zeros(0, np.uint64), 1, 0)
    add_pairs("twin3", np.zeros(0, np.uint64), 3, 0)
    add_pairs("twins_after_giant", from_sizes(lay, [4096], dup=5), 2, 1)
    cx = chain32(min(64, max(len(v) for v in step_classes(lay).values())), 1234, lay)
    add_pairs("twins_after_flag", np.zeros(0, np.uint64), 1, 0, lead=cx, pinned=U(G(0)) | cx)

    # ---- cuts -----------------------------------------------------------------------------------------------------
    add("last_head_at_2047", "cuts", from_sizes(lay, [2047, 5, 30]))
    add("last_head_at_1", "cuts", from_sizes(lay, [1, 2060, 4]))
    add("group_2048_then_more", "cuts", from_sizes(lay, [2048, 7]))
    add("group_2048_ends_data", "cuts", from_sizes(lay, [5, 2048]))
    add("group_2048_alone", "cuts", from_sizes(lay, [2048]))
    add("groups_2047_2049", "cuts", from_sizes(lay, [2047, 3, 2049, 4]))
    # five chunks: heads exactly at 2048 and 8192, at 4095 but not 4096, at 6145 but not 6144
    sizes = [48] * 42 + [32, 50] + [50] * 39 + [47, 52] + [50] * 39 + [48, 52] + [50] * 39 + [45] + [50] * 30
    ends = np.cumsum(sizes)
    assert {2048, 4095, 6145, 8192} <= set(ends.tolist()) and not {4096, 6144} & set(ends.tolist())
    add("heads_around_nominal_ends", "cuts", from_sizes(lay, sizes), max_n=5 * TILE)
    add("chunk_inside_a_giant", "cuts", from_sizes(lay, [40] * 25 + [5000] + [40] * 100), max_n=5 * TILE)
    sizes = [40] * 50 + [48 + 511] + [40] * 37 + [57 + 512] + [40] * 38 + [16 + 513] + [40] * 30
    ends = np.cumsum(sizes)
    assert {2048 + 511, 4096 + 512, 6144 + 513} <= set(ends.tolist())
    add("first_head_511_512_513_in", "cuts", from_sizes(lay, sizes))
    add("giant_ends_at_nominal_end", "cuts", from_sizes(lay, [50] * 10 + [3596] + [50] * 20))
    add("giant_ends_beyond_nominal_end", "cuts", from_sizes(lay, [50] * 10 + [3700] + [50] * 20))
    k = from_sizes(lay, [30] * 100)
    add("bound_seven_times", "cuts", k, max_n=7 * len(k))

    # ---- giant groups ---------------------------------------------------------------------------------------------
    add("giant_nulls", "giant groups", np.concatenate([np.full(3000, G(0), np.uint64), from_sizes(lay, [5, 9], first_group=1)]))
    tok = np.arange(5000); head = np.zeros(5000, bool)
    tok[2048] = tok[2047]; tok[4096] = tok[4095]; tok[2049] = tok[100]; tok[4100] = tok[2040]
    add("giant_round_boundary_dups", "giant groups", np.concatenate([from_heads(lay, head, tok), from_sizes(lay, [6], first_group=1)]))
    for m in (4096, 4097):
        p = one_partition_keys(G(0), 3, 0, m, lay)
        add("giant_partition_%d" % m, "giant groups", np.concatenate([p, p[:4200 - m], from_sizes(lay, [3], first_group=1)]), settle_it=False)
    for ln in (65_536, 65_537):
        tok = np.arange(ln) % 30_011
        g = U(G(0)) | U(1 << lay.nn) | (((tok.astype(np.uint64) * U(0x9E3779B1)) & U((1 << lay.umi_bits) - 1)) << U(2)) | U(3)
        add("giant_%d" % ln, "giant groups", np.concatenate([g, from_sizes(lay, [3], first_group=1)]), settle_it=False)

    # ---- chains ---------------------------------------------------------------------------------------------------
    cap = max(len(v) for v in step_classes(lay).values())
    for m in ((62, 63, 64, 200) if cap >= 200 else (cap,)):     # (10 bases: a step class has fewer than 20 values of hi)
        for rank in (0, 37):
            front = from_sizes(lay, [9] * rank) if rank else np.zeros(0, np.uint64)
            c = U(G(rank)) | chain32(m, 3000 + m, lay)
            grp = np.concatenate([c[:m // 2], c[:7], np.full(3, G(rank), np.uint64), c[m // 2:], c[-2:]])   # copies and NULLs beside it
            add("chain%d_rank%d" % (m, rank), "chains", np.concatenate([front, grp, from_sizes(lay, [9] * 20, first_group=rank + 1)]), pinned=c)
    classes = step_classes(lay)
    steps = sorted(classes, key=lambda s: -len(classes[s]))[:2]
    m = min(63, len(classes[steps[1]]))

    def two_chains(t):
        a = U(G(3)) | chain32(m, 500, lay, step=steps[0]); b = U(G(5)) | chain32(m, 4500 + 61 * t, lay, step=steps[1])
        keys = np.concatenate([from_sizes(lay, [9] * 3), a, from_sizes(lay, [9], first_group=4), b, b[:5], from_sizes(lay, [9] * 5, first_group=6)])
        return settle(keys, len(keys), lay, np.concatenate([a, b]))
    add("two_chains", "chains", first_clean(two_chains), settle_it=False)
    # a key whose walk passes the home of a key with the same hi: only the probe number in the word keeps them apart.
    # C takes B's home, A its own, B walks over A's home.  Five windows, the three in different waves each time; the rest
    # of each window are single heads and NULL keys, which never reach the set, so every order of the three is run.
    parts, pinned, first = [], [], 0
    P = TILE
    places = [(1, 70, 140, 200), (1, 300, 560, 590), (300, 1, 590, 560), (10, 20, 30, 40), (520, 260, 5, 599)]   # C, A, B, B again
    for wv in range(5):
        head = np.ones(P, bool); tok = np.arange(P); tok[::5] = -1
        tok[np.arange(P) % WAVE == WAVE - 1] = -1        # (a head at lane 63 is no single: it would probe)
        tok[P - 2:] = -1                                 # (nor is the last head below a cut)
        head[0:600] = False; tok[0:600] = -1             # rank 0: NULL keys but for the three and a copy of B
        xA = lay.x_of(40_000 + wv)
        s0, step, _ = slot32(xA, 0)
        hiA = xA >> LO32
        xB = (hiA << LO32) | (((s0 - step) ^ (umul24(hiA, 0x9E3779) >> 8)) & (TAB32 - 1))          # home: one step in front of A's
        hiC = [h for h in classes[step] if h != hiA][wv]
        xC = (hiC << LO32) | (((s0 - step) ^ (umul24(hiC, 0x9E3779) >> 8)) & (TAB32 - 1))          # B's home and step
        k = from_heads(lay, head, tok, first_group=first)
        g0 = U(G(first))
        for p, x in zip(places[wv], (xC, xA, xB, xB)):
            k[p] = g0 | U(x)
        pinned += [int(g0) | x for x in (xA, xB, xC)]
        first += int(head.sum())
        parts.append(k)
    add("walk_over_same_hi", "chains", np.concatenate(parts), pinned=pinned)
    return F


_CACHE = {}


def fixtures(lay=L12):
    """name -> Fixture, built once per layout and never changed"""
    if id(lay) not in _CACHE:
        _CACHE[id(lay)] = _fixtures(lay)
    return _CACHE[id(lay)]


def reference_rows(fx):
    """the independent reference of a fixture's rows: sortreduce_ref.want_rows (np.unique, knows nothing of windows)"""
    return want_rows(fx.keys, fs=fx.lay.fs, cs=fx.lay.cs, feat_bits=fx.lay.feat_bits)
