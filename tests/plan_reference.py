"""A plain restatement of the tile-balance plan (k_tile_plan, rt_trace.hip) in Python integers: one
tile at a time, in tile order, no threads, no runs, no scans, no LDS. tests/test_plan_reference.py checks its
properties on the CPU and tests/test_gpu_tile_plan.py compares the kernel with it word for word through
rt_tile_plan_probe.

The rule, as restated here. A cost map holds two words per tile: w, the ticks (10 ns) of the tile's last whole wave,
bit 31 set when parts of a split ran since; and p, the costliest part of its last split (ticks << 2 | layout, layout
1..3; 0: never split). The plan keeps w capped at 16 bits and the part in 80-ns units capped at 13 bits (plan_pack).
A tile's current cost `cur` is w, or with bit 31 and a part the whole estimated from the part (x 20/11, 20/7, 1/0.21
in 10-bit fixed point), capped at 16 bits. L = sum(cur) / slots, mx = max(cur). The list is the plain order unless
mx > 1.25 L and mx > L + min_gain. Then T = max(L, the finest split's floor), raised by a quarter until the parts
fit extra_cap; a tile above T takes the coarsest layout whose estimated part fits T, unless its last split measured
a part above 0.8 x its (stale, capped) whole time w. With 16 measured splits above 0.8 of the raw whole time and none
below, nothing splits (coherent). Items estimated above (L * front) >> 4 form the front class, which goes first;
each class in tile order, a tile's parts consecutive.

Wherever the kernel holds a product or a sum in 32 bits the reference asserts that the value fits, so an input that
would wrap in the kernel is rejected here instead of diverged on.

`mutant` switches one rule to a near miss (MUTANTS): the CPU tests use them to show that the committed cases tell
each rule from its neighbour. The unmutated reference is mutant=None."""
import numpy as np

PLAN_MAX_TILES = 32 * 1024
PLAN_THREADS = 1024
NO_SPLIT = 0xFFFFFFFF  # the threshold of a plan that splits nothing

MUTANTS = (
    "part_12_20",      # the 4-part estimate 11/20 -> 12/20
    "rule08_ge",       # the 0.8 rule's > -> >=
    "inv_1861",        # the inverse constant 1862 -> 1861
    "front_ge",        # e > TF -> >=
    "no_min_gain",     # min_gain ignored
    "useless_17",      # useless >= 16 -> >= 17
    "ignore_since",    # the bit-31 estimate ignored (cur = w always)
    "no_quant",        # the part's 80-ns quantisation dropped
    "front_shift3",    # (L * front) >> 4 -> >> 3
    "t_half",          # T / 4 -> T / 2
    "census_swapped",  # the census on quantised ticks, the 0.8 rule on raw ones
    "no_cap16",        # the 16-bit cap removed
)


def _u32(x, what):
    assert 0 <= x < (1 << 32), f"{what} = {x} does not fit the kernel's 32 bits"
    return x


def split_parts(code):
    return (1, 4, 16, 64)[code]


# --- the storage map ------------------------------------------------------------------------------------------------
def plan_groups(cap, wl):
    """Workgroups of a launch over a list of `cap` items, wl waves each."""
    return -(-cap // wl)


def plan_xwords(cap, wl):
    """Words the XCD-major storage spans: 8 equal slices of whole workgroups."""
    return -(-plan_groups(cap, wl) // 8) * 8 * wl


def plan_xaddr(p, wl, groups):
    """Where list position p is stored. Position p is read by wave p % wl of workgroup k = p // wl; workgroups go
    round robin over 8 XCDs, so workgroup k is XCD k % 8's (k // 8)-th, and each XCD's workgroups lie together."""
    k, j = divmod(p, wl)
    per_xcd = -(-groups // 8)
    xcd, nth = k % 8, k // 8
    return (xcd * per_xcd + nth) * wl + j


# --- cost words -----------------------------------------------------------------------------------------------------
def plan_pack(w, p):
    """The snapshot word of a tile: whole time (16 bits, capped) | part (13 bits of 80-ns units, capped, then its
    layout) << 16 | the "parts ran since" bit."""
    wt = w & 0x7FFFFFFF
    w16 = min(wt, 0xFFFF)
    p15 = ((min(p >> 5, 0x1FFF) << 2) | (p & 3)) if p else 0
    return w16 | (p15 << 16) | (w & 0x80000000)


def _tile(w_raw, p_raw, mutant):
    """(w, has_part, layout, part ticks, since) of a tile as the plan sees it."""
    if p_raw:
        assert 1 <= (p_raw & 3) <= 3, "a non-zero part word carries layout 1..3 (the recording kernel's format)"
    c = plan_pack(w_raw, p_raw)
    w, p15, since = c & 0xFFFF, (c >> 16) & 0x7FFF, c >> 31
    pt = (p15 >> 2) << 3
    if mutant == "no_cap16":
        w = w_raw & 0x7FFFFFFF
    if mutant == "no_quant" and p_raw:
        pt = min(p_raw >> 2, 0x1FFF << 3)
    return w, p15 != 0, p15 & 3, pt, since


def _cur(tile, mutant):
    w, has, lay, pt, since = tile
    if not since or not has or mutant == "ignore_since":
        return w
    inv = {1: 1861 if mutant == "inv_1861" else 1862, 2: 2926, 3: 4876}[lay]
    e = _u32(pt * inv, "pt * inverse") >> 10
    return e if (e < 0xFFFF or mutant == "no_cap16") else 0xFFFF


def _pick(a, split, tile, cur, T, mutant):
    """(layout code, estimated time of the tile's longest item, the layout before the 0.8 rule)."""
    w, has, lay, pt, _ = tile
    kmax = a["kmax_code"]
    n4 = 12 if mutant == "part_12_20" else 11
    code = 0
    if split and kmax and cur > T:
        t20 = _u32(T * 20, "T * 20")
        if kmax == 1 or _u32(cur * n4, "cur * 11") <= t20:
            code = 1
        elif kmax == 2 or _u32(cur * 7, "cur * 7") <= t20:
            code = 2
        else:
            code = 3
    wanted = code
    if code and has:
        if mutant == "census_swapped":
            pass  # judged by the caller on raw ticks
        elif (_u32(pt * 5, "pt * 5") >= w * 4) if mutant == "rule08_ge" else (_u32(pt * 5, "pt * 5") > w * 4):
            code = 0
    if code == 0:
        est = cur
    elif has and lay == code:
        est = pt
    else:
        est = (cur * n4 // 20, cur * 7 // 20, (cur * 215) >> 10)[code - 1]
    return code, est, wanted


def plan_forced(a, t):
    """Forced layouts: 1 every tile in 4, 2 in 16, 4 in 64, 3 by tile position (tx + 2 ty) % 3; capped by kmax."""
    f = a["force"]
    code = {1: 1, 2: 2, 4: 3}.get(f, 0)
    if f == 3:
        fr = t % a["waves_per_frame"]
        wg, wv = divmod(fr, a["wl"])
        tx = (wg % a["grid_x"]) * a["wx"] + wv % a["wx"]
        ty = (wg // a["grid_x"]) * a["wy"] + wv // a["wx"]
        code = (tx + 2 * ty) % 3
    return min(code, a["kmax_code"])


def plan_reference(a, cost, mutant=None):
    """a: the PlanArgs knobs (dict); cost: 2 * ntiles words. Returns a dict: items (the list in order), stats (the
    PlanStats fields the plan decides), cleared (tiles whose part word the plan zeroes), branches (which rules the
    case exercised: the CPU tests' census)."""
    assert mutant is None or mutant in MUTANTS
    n, extra_cap, slots = a["ntiles"], a["extra_cap"], a["slots"]
    assert 1 <= n <= PLAN_MAX_TILES and a["wl"] >= 1 and a["kmax_code"] <= 3 and a["force"] <= 4
    cost = [int(x) for x in cost]
    assert len(cost) == 2 * n
    cap = _u32(n + extra_cap, "ntiles + extra_cap")
    force, branches = a["force"], set()
    split = a["split"] != 0
    T, mx, L, want, total, tail = NO_SPLIT, 0, 0, 0, 0, False
    tiles, cur = [], []
    raw_rule08 = {}

    if not force:
        useless = useful = 0
        lane_sum = [0] * PLAN_THREADS  # thread i of the kernel sums tiles i, i + 1024, ...: at most 32 of them
        for t in range(n):
            w_raw, p_raw = cost[2 * t], cost[2 * t + 1]
            tl = _tile(w_raw, p_raw, mutant)
            c = _cur(tl, mutant)
            tiles.append(tl)
            cur.append(c)
            lane_sum[t % PLAN_THREADS] += c
            wx = w_raw & 0x7FFFFFFF
            if wx > 0xFFFF:
                branches.add("whole_capped")
            if (p_raw >> 5) > 0x1FFF:
                branches.add("part_capped")
            if tl[4] and tl[1]:
                branches.add("cur_from_parts")
            # the census of measured splits, on raw ticks
            if p_raw and wx:
                if mutant == "census_swapped":
                    bad = tl[3] * 5 > tl[0] * 4
                    raw_rule08[t] = (p_raw >> 2) * 5 > wx * 4
                else:
                    bad = (p_raw >> 2) * 5 > wx * 4
                if bad:
                    useless += 1
                else:
                    useful += 1
            elif mutant == "census_swapped" and p_raw:
                raw_rule08[t] = True
        _u32(max(lane_sum), "a thread's sum of times")
        total, mx = sum(cur), max(cur)
        if useless >= (17 if mutant == "useless_17" else 16) and useful == 0:
            if split:
                branches.add("coherent")
            split = False
        L = _u32(total // (slots if slots else 1), "L")
        gain = 0 if mutant == "no_min_gain" else a["min_gain"]
        tail = mx * 4 > L * 5 and mx > _u32(L + gain, "L + min_gain")

    def pick(t, thr):
        code, est, wanted = _pick(a, split, tiles[t], cur[t], thr, mutant)
        if mutant == "census_swapped" and code and raw_rule08.get(t, False):
            code, est = 0, cur[t]
        return code, est, wanted

    if tail:
        F = (mx * 215) >> 10 if a["kmax_code"] >= 3 else (mx * 7) // 20
        T = max(L, F)
        if split:
            cand = [t for t in range(n) if cur[t] > T]  # T only rises: the tiles above it only shrink
            raises = 0
            while True:
                tot = sum(split_parts(pick(t, T)[0]) - 1 for t in cand)
                if raises == 0:
                    want = min(tot, 0xFFFFFFFF)
                if tot <= extra_cap:
                    break
                # T >= 0.21 mx and 0.21 x 1.25^7 > 1: after 7 raises no tile exceeds T, so the kernel's iteration-23
                # last resort and its T >= 65535 escape are never reached
                raises += 1
                assert raises <= 7 and T < 65535, "the budget loop raises T at most 7 times"
                T = T + T // (2 if mutant == "t_half" else 4) + 1
                cand = [t for t in cand if cur[t] > T]
            if raises:
                branches.add("T_raised")

    items, cleared = list(range(0, n << 8, 1 << 8)), set()
    nsplit = nitems = refused = 0
    nitems, pays = n, False
    if force or tail:
        TF = NO_SPLIT
        if not force and a["front"]:
            TF = _u32(L * a["front"], "L * front") >> (3 if mutant == "front_shift3" else 4)
        front, back = [], []
        for t in range(n):
            if force:
                code, est, wanted = plan_forced(a, t), 0, 0
            else:
                code, est, wanted = pick(t, T)
            fr = (not force) and (est >= TF if mutant == "front_ge" else est > TF)
            (front if fr else back).append((t, code))
            if code:
                nsplit += 1
                branches.add(f"code{code}")
                if not force:
                    cleared.add(t)
                    if tiles[t][1] and tiles[t][2] == code:
                        branches.add("est_from_part")
            elif wanted:
                branches.add("kept_whole_08")
        items = []
        for cls in (front, back):
            for t, code in cls:
                first = (t << 8) | code  # then part q in bits 2..7
                items.extend(range(first, first + (split_parts(code) << 2), 4))
        nfront_items = sum(split_parts(code) for _, code in front)
        if a["prio"]:
            items[:nfront_items] = [it | 0x80000000 for it in items[:nfront_items]]
        refused = max(0, len(items) - cap)
        nitems = min(len(items), cap)
        pays = nsplit > 0 or (n > slots and 0 < len(front) < n)
        if pays:
            branches.add("pays_split" if nsplit else "pays_front")
    else:
        branches.add("no_tail")
    if refused:
        branches.add("refused")
        items, nitems, nsplit, pays = list(range(0, n << 8, 1 << 8)), n, 0, False
    assert len(items) == nitems or refused
    stats = {
        "nitems": nitems, "nsplit": nsplit, "want_extra": want, "max_cost": mx, "mean_cost": total // n,
        "threshold": T, "pays": int(pays), "coherent": int(not force and a["split"] != 0 and not split),
        "refused": refused, "refused_plans": int(refused > 0), "slots": slots,
    }
    return {"items": items, "stats": stats, "cleared": cleared, "branches": branches, "L": L}


# --- the committed cases (shared by the CPU and the GPU test) -------------------------------------------------------
NTILES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 5000, 32767, 32768)
KNOBS = ("ntiles", "extra_cap", "slots", "kmax_code", "force", "split", "front", "prio", "min_gain",
         "waves_per_frame", "grid_x", "wx", "wy", "wl")


def _args(n, **kw):
    a = dict(ntiles=n, extra_cap=n // 8 + 64, slots=7168, kmax_code=3, force=0, split=1, front=8, prio=1,
             min_gain=1000, waves_per_frame=n, grid_x=max(1, n // 8), wx=2, wy=2, wl=4)
    a.update(kw)
    assert set(a) == set(KNOBS)
    return a


def _part(rng, whole, frac, layout):
    """A part word: the costliest part took frac of the whole time."""
    ticks = np.maximum(1, (whole.astype(np.float64) * frac).astype(np.int64))
    return ((ticks << 2) | layout).astype(np.uint32)


def _heavy(rng, n, share):
    k = max(1, int(n * share))
    return rng.choice(n, size=min(k, n), replace=False)


def gen_costs(kind, n, rng, a):
    """A seeded cost map of `kind` for the knobs in a (which it may adjust: slots, extra_cap, min_gain)."""
    w = rng.integers(1500, 2600, size=n).astype(np.int64)
    p = np.zeros(n, dtype=np.uint32)
    since = np.zeros(n, dtype=bool)
    if kind == "flat":
        a["slots"] = max(1, n // 2)  # L about twice the mean: no tile outlasts it
    elif kind == "flat_gain":
        # a tail by the ratio (mx > 1.25 L) that min_gain rejects (mx <= L + min_gain)
        a["slots"] = max(1, n)
        w[_heavy(rng, n, 0.02)] = 3400
        a["min_gain"] = 2500
    elif kind in ("tail", "budget", "tiny_slots"):
        share = {"tail": 0.03, "budget": 0.08, "tiny_slots": 0.03}[kind]
        hv = _heavy(rng, n, share)
        w[hv] = rng.integers(12000, 64000, size=hv.size)
        a["slots"] = max(1, n // 3) if kind != "tail" else max(1, min(7168, n // 2))
        if kind == "budget":
            a["extra_cap"] = max(3, n // 64)
        # measured parts on some heavy tiles, layouts 1..3, 0.15 .. 0.95 of the whole; half of them ran since
        m = hv[: max(1, (2 * hv.size) // 3)]
        lay = rng.integers(1, 4, size=m.size)
        frac = rng.uniform(0.15, 0.95, size=m.size)
        p[m] = _part(rng, w[m], frac, lay)
        since[m[::2]] = True
        # and on a few light tiles (useful splits long ago)
        lt = _heavy(rng, n, 0.01)
        lt = lt[p[lt] == 0]
        p[lt] = _part(rng, w[lt], rng.uniform(0.2, 0.6, size=lt.size), rng.integers(1, 4, size=lt.size))
    elif kind == "coherent":
        hv = _heavy(rng, n, 0.03)
        w[hv] = rng.integers(12000, 60000, size=hv.size)
        a["slots"] = max(1, n // 3)
        m = _heavy(rng, n, max(0.05, 24.0 / n))  # at least 16 where n allows
        p[m] = _part(rng, w[m], rng.uniform(0.82, 0.99, size=m.size), rng.integers(1, 4, size=m.size))
    elif kind == "saturated":
        w = rng.integers(15000, 30000, size=n).astype(np.int64)
        hv = _heavy(rng, n, 0.02)
        w[hv] = rng.integers(70000, 400000, size=hv.size)  # above 0xffff
        a["slots"] = n  # L about the mean: many tiles above the first threshold, so the budget loop has work
        m = hv[: max(1, hv.size // 2)]
        p[m] = _part(rng, w[m], rng.uniform(0.3, 0.9, size=m.size), rng.integers(1, 4, size=m.size))  # some above 13 bits
        since[m[::2]] = True
    else:
        raise ValueError(kind)
    cost = np.zeros(2 * n, dtype=np.uint32)
    cost[0::2] = w.astype(np.uint32) | (since.astype(np.uint32) << 31)
    cost[1::2] = p
    return cost


def _edge_cases():
    """Hand-made maps that sit exactly on a rule's boundary (the mutants' discriminators). 64 light tiles of 1000
    ticks and a few special ones; slots 16, so L = total / 16."""
    out = []

    def case(name, special, **kw):
        n = 64
        w = [1000] * n
        p = [0] * n
        for k, (wt, pt) in enumerate(special):
            w[k * 5 + 1], p[k * 5 + 1] = wt, pt
        cost = np.zeros(2 * n, dtype=np.uint32)
        cost[0::2], cost[1::2] = w, p
        a = _args(n, slots=16, min_gain=0, **kw)
        out.append((f"edge-{name}", a, cost))

    # 0.8 rule exactly met: part 16000 of whole 20000 (5 pt == 4 w): still split; 16008: kept whole
    case("rule08-eq", [(20000, (16000 << 2) | 1), (20000, (16008 << 2) | 1), (30000, 0)], kmax_code=2)
    # the inverse constant: the costliest tile's cost comes from its part (8000 ticks, layout 1 -> 14546)
    case("inv-const", [(0x80000000 | 9000, (8000 << 2) | 1), (9000, 0)], kmax_code=2)
    # the same tile ignoring bit 31 would cost 2000
    case("since", [(0x80000000 | 2000, (8000 << 2) | 2), (9000, 0)], kmax_code=3)
    # raw against quantised ticks: part 8007 of 10000 (raw above 0.8, quantised 8000 not), 17 such tiles below
    case("quant", [(10000, (8007 << 2) | 1), (40000, 0)], kmax_code=1)
    # whole times above 16 bits: the cap decides L and the largest cost
    case("cap16", [(200000, 0), (70000, (300000 << 2) | 2), (0x80000000 | 5000, (40000 << 2) | 3)], kmax_code=3)
    # 11/20: T = 0.35 x 40000 = 14000; a tile of 25000: 11/20 -> 13750 fits (4 parts), 12/20 -> 15000 does not (16)
    case("part-11-20", [(40000, 0), (25000, 0), (25400, 0)], kmax_code=2)
    return out


def _edge_front_cases():
    """Tiles whose estimate equals the front threshold (L * front) >> 4 exactly, one tick above it, and the same
    around (L * front) >> 3. One tile absorbs the difference, so the total (and with it L) is chosen first."""
    out = []
    for front, n in ((8, 64), (5, 96)):
        slots, total = 8, 8 * 25000 + 3
        L = total // slots
        tf, tf3 = (L * front) >> 4, (L * front) >> 3
        w = [1000] * n
        w[3] = 40000  # the tail (never split: split = 0)
        w[10], w[11], w[12], w[13] = tf, tf + 1, tf3, tf3 + 1
        w[20] = 0
        w[20] = total - sum(w)
        assert 0 < w[20] < 40000 and sum(w) == total
        cost = np.zeros(2 * n, dtype=np.uint32)
        cost[0::2] = w
        out.append((f"edge-front{front}", _args(n, slots=slots, min_gain=0, split=0, front=front), cost))
    return out


def _coherent_edge_cases():
    """Exactly 16 and exactly 17 useless measured splits, none useful; and 16 useless with one useful."""
    out = []
    for name, nbad, ngood in (("16", 16, 0), ("17", 17, 0), ("16+1", 16, 1), ("15", 15, 0)):
        n = 128
        w = [2000] * n
        p = [0] * n
        w[5] = 30000
        w[6] = 28000
        for k in range(nbad):
            w[20 + k] = 6000
            p[20 + k] = (5400 << 2) | (1 + k % 3)
        for k in range(ngood):
            p[60 + k] = (800 << 2) | 1
        cost = np.zeros(2 * n, dtype=np.uint32)
        cost[0::2], cost[1::2] = w, p
        out.append((f"edge-coherent{name}", _args(n, slots=32, min_gain=0), cost))
    # raw against quantised in the census: 16 parts of 8007 / 10000 (raw above 0.8, quantised exactly 0.8)
    n = 128
    w = [2000] * n
    p = [0] * n
    w[5] = 50000
    for k in range(16):
        w[20 + k] = 10000
        p[20 + k] = (8007 << 2) | 1
    cost = np.zeros(2 * n, dtype=np.uint32)
    cost[0::2], cost[1::2] = w, p
    out.append(("edge-census-raw", _args(n, slots=32, min_gain=0, kmax_code=1), cost))
    return out


def plan_cases():
    """The committed case list: (name, knobs, cost words). Deterministic."""
    cases = []
    kinds = ("flat", "flat_gain", "tail", "coherent", "saturated", "budget", "tiny_slots")
    k = 0
    for n in NTILES:
        for kind in kinds:
            if kind in ("coherent", "tiny_slots", "flat_gain") and n < 63:
                continue
            for rep in range(2 if n <= 5000 else 1):
                k += 1
                rng = np.random.default_rng(1000 + k)
                # the knobs rotate with the case index, so every value meets every kind and size class
                wl = (1, 4)[k % 2]
                a = _args(n, kmax_code=(3, 2, 1, 3, 0, 3, 2)[k % 7] if kind != "flat" else k % 4,
                          wl=wl, front=(8, 0, 8)[k % 3], prio=(k // 2) % 2,
                          split=0 if (kind == "tiny_slots" and rep == 0) else (0 if k % 11 == 0 else 1))
                cost = gen_costs(kind, n, rng, a)
                if kind != "budget":
                    # a budget that makes ntiles + extra_cap a multiple of 8 * wl in every other case
                    cap = n + a["extra_cap"]
                    if k % 4 < 2:
                        cap = -(-cap // (8 * wl)) * (8 * wl)
                    elif cap % (8 * wl) == 0:
                        cap += 1
                    a["extra_cap"] = cap - n
                cases.append((f"{kind}-n{n}-{rep}", a, cost))
    # code 3 (64 parts) is the rare layout: one dominant tile, a generous budget
    for j, n in enumerate((2, 64, 65, 1025, 2049, 5000)):
        rng = np.random.default_rng(5000 + j)
        a = _args(n, kmax_code=3, slots=max(1, n // 2), extra_cap=4 * n + 64, wl=(1, 4)[j % 2], prio=j % 2)
        cost = gen_costs("flat", n, rng, dict(a))
        hv = _heavy(rng, n, 0.02)
        cost[2 * hv] = rng.integers(50000, 65000, size=hv.size)
        cases.append((f"fine-n{n}", a, cost))
    # forced layouts (the costs are not read); a budget too small for the parts: refused, the identity list
    for j, (force, n, kmax) in enumerate(((1, 65, 3), (2, 1025, 3), (3, 2049, 2), (4, 63, 3), (3, 64, 3), (2, 5000, 1),
                                          (1, 32768, 3), (4, 1024, 3))):
        wl = (4, 1)[j % 2]
        most = {1: 4, 2: 16, 3: 16, 4: 64}[force]
        a = _args(n, force=force, kmax_code=kmax, extra_cap=(most - 1) * n, wl=wl, wx=2 if wl == 4 else 1,
                  wy=2 if wl == 4 else 1, grid_x=7, waves_per_frame=max(1, n // 2))
        rng = np.random.default_rng(7000 + j)
        cases.append((f"forced{force}-n{n}", a, gen_costs("tail", n, rng, dict(a))))
    for j, (force, n) in enumerate(((2, 1025), (1, 64), (4, 2047), (3, 5000))):
        a = _args(n, force=force, extra_cap=(64, 3, 1000, 17)[j], wl=(4, 1)[j % 2], wx=(2, 1)[j % 2], wy=(2, 1)[j % 2],
                  grid_x=5, waves_per_frame=n)
        rng = np.random.default_rng(7100 + j)
        cases.append((f"forced{force}-refused-n{n}", a, gen_costs("tail", n, rng, dict(a))))
    cases += _edge_cases() + _edge_front_cases() + _coherent_edge_cases()
    return cases
