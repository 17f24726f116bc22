"""The plan reference (tests/plan_reference.py) on its own, no GPU: every list it returns is a cover in the promised
order, the committed cases reach every branch of the rule, and they tell each rule from its nearest wrong
neighbour (the reference's single-rule mutants). tests/test_gpu_tile_plan.py then holds k_tile_plan to this
reference on the same cases."""
import collections

import pytest

import plan_reference as pr

CASES = pr.plan_cases()
NAMES = [name for name, _, _ in CASES]


@pytest.fixture(scope="module")
def results():
    """The unmutated reference of every committed case, computed once and left unchanged."""
    return [pr.plan_reference(a, cost) for _, a, cost in CASES]


def identity(n):
    return [t << 8 for t in range(n)]


def test_case_list_spans_the_parameters():
    assert len(NAMES) == len(set(NAMES))
    args = [a for _, a, _ in CASES]
    assert {a["ntiles"] for a in args} >= set(pr.NTILES)
    for key, want in (("kmax_code", {0, 1, 2, 3}), ("wl", {1, 4}), ("front", {0, 8}), ("prio", {0, 1}),
                      ("split", {0, 1}), ("force", {0, 1, 2, 3, 4})):
        assert {a[key] for a in args} >= want, key
    # every size meets wl 1 and 4, prio on and off, and a budget that does and does not fill the storage's slices
    for n in pr.NTILES:
        mine = [a for a in args if a["ntiles"] == n and not a["force"]]
        assert {a["wl"] for a in mine} == {1, 4}, n
        assert {a["prio"] for a in mine} == {0, 1}, n
        assert {(a["ntiles"] + a["extra_cap"]) % (8 * a["wl"]) == 0 for a in mine} == {True, False}, n
    # the cost words obey the recording kernel's format
    for name, a, cost in CASES:
        p = cost[1::2]
        assert (((p & 3) != 0) | (p == 0)).all(), name


def test_every_list_is_a_cover_in_class_and_tile_order(results):
    for (name, a, _), r in zip(CASES, results):
        n, items, st = a["ntiles"], r["items"], r["stats"]
        assert st["nitems"] == len(items) <= n + a["extra_cap"], name
        seen = collections.defaultdict(list)
        for it in items:
            assert (it >> 8) & 0x7FFFFF < n, name
            seen[(it >> 8) & 0x7FFFFF].append(((it >> 2) & 63, it & 3))
        assert len(seen) == n, name
        for t, parts in seen.items():
            codes = {c for _, c in parts}
            assert len(codes) == 1, (name, t)
            assert [q for q, _ in parts] == list(range(pr.split_parts(codes.pop()))), (name, t)
        assert st["nsplit"] == sum(1 for parts in seen.values() if parts[0][1] != 0), name
        # two classes, the front one first; each in ascending tile order, a tile's parts consecutive
        order = [(it >> 8) & 0x7FFFFF for it in items[:: 1]]
        firsts = [t for k, t in enumerate(order) if k == 0 or order[k - 1] != t]
        assert len(firsts) == n, name  # consecutive parts: each tile starts once
        drops = [k for k in range(1, n) if firsts[k] < firsts[k - 1]]
        assert len(drops) <= 1, name
        flagged = [bool(it >> 31) for it in items]
        if a["prio"] and not a["force"] and not st["refused"]:
            nfront = sum(flagged)
            assert flagged == [True] * nfront + [False] * (len(items) - nfront), name
            if drops:  # the flag ends exactly where the back class begins
                start_of_back = order.index(firsts[drops[0]])
                assert nfront == start_of_back, name
        else:
            assert not any(flagged), name
        if st["pays"]:
            assert items != identity(n), name
        assert r["cleared"] == ({t for t, parts in seen.items() if parts[0][1]} if not a["force"] else set()) or \
            st["refused"], name


def test_no_tail_and_refusal_give_the_identity_list(results):
    seen_no_tail = seen_refused = 0
    for (name, a, _), r in zip(CASES, results):
        if "no_tail" in r["branches"]:
            seen_no_tail += 1
            assert r["items"] == identity(a["ntiles"]) and not r["cleared"], name
            assert r["stats"]["threshold"] == pr.NO_SPLIT and r["stats"]["pays"] == 0, name
        if "refused" in r["branches"]:
            seen_refused += 1
            assert r["items"] == identity(a["ntiles"]), name
            assert r["stats"]["nsplit"] == 0 and r["stats"]["pays"] == 0 and r["stats"]["refused_plans"] == 1, name
    assert seen_no_tail and seen_refused


BRANCHES = ("no_tail", "coherent", "T_raised", "code1", "code2", "code3", "kept_whole_08", "est_from_part",
            "cur_from_parts", "whole_capped", "part_capped", "pays_split", "pays_front", "refused")


def test_branch_census(results):
    census = collections.Counter()
    for r in results:
        census.update(r["branches"])
    assert set(census) <= set(BRANCHES)
    for b in BRANCHES:
        assert census[b] >= 3, (b, dict(census))
    # the adaptive cases alone reach the three layouts too (the forced ones do by construction)
    adaptive = collections.Counter()
    for (_, a, _), r in zip(CASES, results):
        if not a["force"]:
            adaptive.update(r["branches"])
    for b in ("code1", "code2", "code3"):
        assert adaptive[b] >= 3, (b, dict(adaptive))


@pytest.mark.parametrize("mutant", pr.MUTANTS)
def test_cases_tell_each_rule_from_its_neighbour(results, mutant):
    """At least one committed case gives another result under the mutant (another list, other stats, other cleared
    tiles, or a value the mutant cannot hold in 32 bits). The largest maps are left out: the small ones suffice."""
    killed = []
    for (name, a, cost), base in zip(CASES, results):
        if a["ntiles"] > 5000 or a["force"]:
            continue
        try:
            r = pr.plan_reference(a, cost, mutant)
        except AssertionError:
            killed.append(name)
            continue
        if (r["items"], r["stats"], r["cleared"]) != (base["items"], base["stats"], base["cleared"]):
            killed.append(name)
    assert killed, f"no committed case distinguishes the rule from mutant {mutant}"


def test_plan_pack_and_the_two_current_costs():
    assert pr.plan_pack(0, 0) == 0
    assert pr.plan_pack(1234, 0) == 1234
    assert pr.plan_pack(0x80000000 | 70000, (800 << 2) | 2) == 0x80000000 | 0xFFFF | ((((800 >> 3) << 2) | 2) << 16)
    assert pr.plan_pack(5, (7 << 2) | 1) == 5 | (1 << 16)          # a part below 80 ns keeps its layout
    assert pr.plan_pack(5, (0x7FFFF << 2) | 3) == 5 | (((0x1FFF << 2) | 3) << 16)  # the 13-bit cap
    # cur: the whole time, or with bit 31 the whole estimated from the part
    cur = lambda w, p: pr._cur(pr._tile(w, p, None), None)  # noqa: E731
    assert cur(9000, (8000 << 2) | 1) == 9000
    assert cur(0x80000000 | 9000, 0) == 9000
    assert cur(0x80000000 | 9000, (8000 << 2) | 1) == (8000 * 1862) >> 10 == 14546
    assert cur(0x80000000 | 9000, (8000 << 2) | 2) == (8000 * 2926) >> 10
    assert cur(0x80000000 | 9000, (8000 << 2) | 3) == (8000 * 4876) >> 10
    assert cur(0x80000000 | 9000, (60000 << 2) | 3) == 0xFFFF
    with pytest.raises(AssertionError):
        pr._tile(100, 8 << 2, None)  # layout 0 with a time: not the recording kernel's format


def test_inputs_that_would_wrap_are_rejected():
    a = pr._args(4, slots=4, front=0x20000)
    with pytest.raises(AssertionError, match="32 bits"):
        pr.plan_reference(a, [60000, 0, 60000, 0, 65000, 0, 1000, 0])
    a = pr._args(4, slots=4, min_gain=0xFFFFFFFF)
    with pytest.raises(AssertionError, match="32 bits"):
        pr.plan_reference(a, [60000, 0, 60000, 0, 65000, 0, 1000, 0])


@pytest.mark.parametrize("wl", [1, 2, 4, 16])
def test_storage_map_is_a_bijection_with_one_slice_per_xcd(wl):
    for cap in (1, 7, 8, 9, 63, 64, 65, 8 * wl, 8 * wl + 1, 1000, 4161):
        groups, words = pr.plan_groups(cap, wl), pr.plan_xwords(cap, wl)
        assert groups * wl >= cap > (groups - 1) * wl and words >= groups * wl and words % (8 * wl) == 0
        addr = [pr.plan_xaddr(p, wl, groups) for p in range(groups * wl)]
        assert len(set(addr)) == len(addr) and min(addr) >= 0 and max(addr) < words
        per = words // 8
        for x in range(8):  # the workgroups with k % 8 == x: one contiguous slice, in workgroup order
            mine = [addr[p] for p in range(groups * wl) if (p // wl) % 8 == x]
            assert mine == list(range(x * per, x * per + len(mine))), (cap, x)
