"""tests/hash_table_cases.py without a GPU: every case is what its name claims under the numpy twin of the device hash (home
slots, cluster extents, duplicate rows, distinct values per wave), and the references agree with a brute-force O(n^2) count.
tests/test_gpu_hash_tables.py pins the twin itself to the device."""
import numpy as np
import pytest

import hash_table_cases as H
from h2util import R_MOD, from_mont


def test_table_capacity_steps():
    assert [H.table_capacity(u) for u in (0, 1, 32, 33, 512, 513)] == [64, 64, 64, 128, 1024, 2048]
    assert H.table_capacity(64) == 128 and H.table_capacity(65) == 256 and H.table_capacity(2 * 250) == 1024


def test_key_hash_twin_on_hand_computed_values():
    """the twin against the same arithmetic in Python integers, including the all-zero key and all-ones limbs"""
    def by_hand(limbs):
        h = 0x9E3779B9
        for l in limbs:
            h ^= l
            h = h * 0x85EBCA6B & 0xFFFFFFFF
            h ^= h >> 13
        h = h * 0xC2B2AE35 & 0xFFFFFFFF
        return h ^ (h >> 16)

    keys = np.concatenate([H.mont([0, 1, R_MOD - 1, 65535]), np.full((1, 4), 2 ** 64 - 1, dtype=np.uint64)])
    keys = np.concatenate([keys] + [np.stack([a, b]) for _, a, b in H.one_limb_pairs()])
    limbs = H.limbs32(keys)
    assert [int(h) for h in H.key_hash(limbs)] == [by_hand([int(x) for x in row]) for row in limbs]
    # least significant limb first
    assert [int(x) for x in H.limbs32(np.array([[1 | 2 << 32, 3, 0, 4 << 32]], dtype=np.uint64))[0]] == [1, 2, 3, 0, 0, 0, 0, 4]


def test_range_table_keys_fill_every_home_slot():
    """what the case builders rely on: the keys of a 16-bit range table give clusters of any needed length on every slot"""
    assert from_mont(H.small_keys()[[0, 1, 65535]]) == [0, 1, 65535]
    by64, by1024 = H.small_by_home(64), H.small_by_home(1024)
    assert len(by64) == 64 and min(len(v) for v in by64.values()) > 900
    assert len(by1024) == 1024 and min(len(v) for v in by1024.values()) >= 37


def test_one_limb_pairs_differ_in_exactly_one_limb():
    pairs = H.one_limb_pairs()
    assert [limb for limb, _, _ in pairs] == list(range(8))
    for limb, a, b in pairs:
        diff = (H.limbs32(a)[0] != H.limbs32(b)[0]).nonzero()[0].tolist()
        assert diff == [limb]
        assert H.key_hash(H.limbs32(a))[0] != H.key_hash(H.limbs32(b))[0]


def _distinct(c):
    return list(dict.fromkeys(H.keys_of(c.table[:c.usable])))


@pytest.mark.parametrize("name", H.NAMES)
def test_cases_are_what_they_are_named(name):
    c = H.case(name)
    cap = H.table_capacity(c.usable)
    assert c.table.shape == (c.n, 4) and c.table.dtype == np.uint64 and c.usable <= c.n
    assert all(a.shape == (c.n, 4) and a.dtype == np.uint64 for a in c.inputs)
    assert all(sum(int(x) << (64 * i) for i, x in enumerate(k)) < R_MOD for k in H.keys_of(c.table))
    assert cap == c.claim["cap"]
    m, misses = H.multiplicities(c.table, c.inputs, c.usable, c.n)
    assert misses == c.claim["misses"] and sum(m) + misses == len(c.inputs) * c.usable
    keys = H.keys_of(c.table)
    first = {}
    for i, k in enumerate(keys[:c.usable]):
        first.setdefault(k, i)
    # rows past usable repeat a value that occurs inside, and are credited nothing
    assert c.usable < c.n and all(k in first for k in keys[c.usable:]) and not any(m[c.usable:])
    # every distinct table value is hit by some input (so also the last one of every probe chain)
    if name not in ("one_limb_pairs_absent", "hot_waves"):
        assert all(m[r] > 0 for r in first.values())
    distinct = np.array(_distinct(c), dtype=np.uint64)
    homes = H.home_slots(distinct, cap)

    if name in ("wrap", "full_cluster_miss", "capacity_step", "adjacent_homes"):
        assert set(homes) == c.claim["homes"]
        assert sorted(H.occupied_slots(c.table[:c.usable], cap)) == sorted(c.claim["occupied"])
    if name in ("wrap", "full_cluster_miss"):
        assert len(distinct) == 32 and sorted(c.claim["occupied"]) == list(range(30)) + [62, 63]
    if name == "full_cluster_miss":
        # one input value is absent, probes slot 62 first and so walks all 32 occupied slots to the empty slot 30
        absent = [k for a in c.inputs for k in H.keys_of(a[:c.usable]) if k not in first]
        assert len(absent) == 1
        assert H.home_slots(np.array(absent, dtype=np.uint64), cap) == [c.claim["absent_home"]] == [62]
    if name == "capacity_step":
        assert c.usable == 33 and cap == 128 and sorted(c.claim["occupied"]) == list(range(31)) + [126, 127]
    if name == "adjacent_homes":
        per_home = {h: homes.count(h) for h in set(homes)}
        assert per_home == {h: 30 for h in range(500, 516)} and c.claim["occupied"] == list(range(500, 980))
        dup_rows = [i for i, k in enumerate(keys[:c.usable]) if first[k] != i]
        assert len(dup_rows) == 32 and all(i - first[keys[i]] > 1 for i in dup_rows)
    if name.startswith("far_duplicates"):
        (a, rows_a), (b, rows_b) = c.claim["duplicates"].items()
        ka, kb = (tuple(int(x) for x in H.small_keys()[v]) for v in (a, b))
        assert [i for i, k in enumerate(keys[:c.usable]) if k == ka] == [5, 300, 301, 700, 1023] == list(rows_a)
        assert [i for i, k in enumerate(keys[:c.usable]) if k == kb] == [255, 256] == list(rows_b)
        assert len({r // 256 for r in rows_a}) == 4 and [r // 256 for r in rows_b] == [0, 1]
        # all credit on rows 5 and 255
        assert m[5] > 8 and m[255] > 8 and not any(m[r] for r in (300, 301, 700, 1023, 256))
        assert len(c.claim["pairs"]) == 150
        for v, (lo, hi) in c.claim["pairs"].items():
            k = tuple(int(x) for x in H.small_keys()[v])
            assert [i for i, kk in enumerate(keys[:c.usable]) if kk == k] == [lo, hi] and hi - lo > 1
            assert m[lo] >= 2 and m[hi] == 0                    # an input hits the value through its HIGHER row's copy too
        assert sum(1 for lo, hi in c.claim["pairs"].values() if lo // 256 != hi // 256) > 50
        assert sum(1 for lo, hi in c.claim["pairs"].values() if lo // 64 != hi // 64 and lo // 256 == hi // 256) > 10
        for dup, others in c.claim["colliders"].items():
            home = H.home_slots(H.small_keys()[[dup]], cap)[0]
            assert H.home_slots(H.small_keys()[others], cap) == [home] * 3
            rows = [keys.index(tuple(int(x) for x in H.small_keys()[v])) for v in others]
            lo, hi = min(c.claim["duplicates"][dup]), max(c.claim["duplicates"][dup])
            assert any(lo < r < hi for r in rows) or (lo, hi) == (255, 256)
            assert any(r < lo for r in rows) and any(r > lo for r in rows)
        assert bool(c.claim["colliders"]) == name.endswith("collision")
    if name == "hot_waves":
        assert c.usable == 250 and c.n == 256 and c.usable % 64
        seen = set()
        for col, counts in zip(c.inputs, c.claim["wave_counts"]):
            ks = H.keys_of(col)
            got = tuple(len(set(ks[w * 64:min(w * 64 + 64, c.usable)])) for w in range(4))
            assert got == tuple(counts)
            seen.update(got)
            for w in range(4):          # uneven shares; with 3 or more values some lanes are left to the individual atomics
                shares = sorted(np.unique(np.array(ks[w * 64:min(w * 64 + 64, c.usable)]), axis=0, return_counts=True)[1])
                assert len(set(shares)) == len(shares)
        assert seen == {1, 2, 3, 5}
        assert any(len(set(H.keys_of(col[:64]))) == 1 for col in c.inputs)      # a whole wave on one row
        assert {counts[3] for counts in c.claim["wave_counts"]} == {1, 2, 3, 5}   # the partial wave sees every count
    if name == "padding":
        p = c.claim["padding_first"]
        assert p == 40 and len(set(keys[:p])) == p and set(keys[p:c.usable]) == {keys[p]} and keys[p] not in keys[:p]
        assert keys[p] == (0, 0, 0, 0)
        assert m[p] > 2 * c.usable and not any(m[p + 1:])
        assert keys[c.usable] == keys[3] and all(H.keys_of(a[c.usable:]) == [keys[3]] * (c.n - c.usable) for a in c.inputs)
    if name.startswith("one_limb_pairs"):
        hand = H.keys_of(H.mont([0, 1, R_MOD - 1]))
        assert keys[:3] == hand
        pairs = c.claim["pairs"]
        base = tuple(int(x) for x in pairs[0][1])
        assert base in first
        present = [tuple(int(x) for x in b) in first for _, _, b in pairs]
        assert present == [name == "one_limb_pairs"] * 8
        if name == "one_limb_pairs":                     # every row's count differs from its neighbours'
            assert len({m[first[tuple(int(x) for x in b)]] for _, _, b in pairs} | {m[first[base]]}) >= 4


def _brute_first_rows(table, col, usable):
    """for each row < usable of `col`: the lowest table row < usable with the same limbs, or -1; O(n^2) by numpy"""
    out = []
    for v in col[:usable]:
        hit = (table[:usable] == v).all(axis=1).nonzero()[0]
        out.append(int(hit[0]) if len(hit) else -1)
    return out


@pytest.mark.parametrize("name", H.NAMES)
def test_references_agree_with_brute_force(name):
    c = H.case(name)
    rows = [_brute_first_rows(c.table, col, c.usable) for col in c.inputs]
    want = [0] * c.n
    for rr in rows:
        for r in rr:
            if r >= 0:
                want[r] += 1
    misses = sum(r < 0 for rr in rows for r in rr)
    assert H.multiplicities(c.table, c.inputs, c.usable, c.n) == (want, misses)
    # a row range, clipped at usable
    lo, hi = c.usable // 3 + 1, c.n
    part = [0] * c.n
    for rr in rows:
        for r in rr[lo:]:
            if r >= 0:
                part[r] += 1
    assert H.multiplicities(c.table, c.inputs, c.usable, c.n, rows=(lo, hi)) == (part, sum(r < 0 for rr in rows for r in rr[lo:]))
    assert H.multiplicities(c.table, c.inputs, c.usable, c.n, rows=(5, 5)) == ([0] * c.n, 0)
    # the first input that misses, per row
    tags = [7 << 16 | j for j in range(len(c.inputs))]
    fails = []
    for row in range(c.usable):
        for j, rr in enumerate(rows):
            if rr[row] < 0:
                fails.append((9, tags[j], row))
                break
    assert H.lookup_failures(c.table, c.inputs, tags, c.usable, index=9) == sorted(fails)
    # shuffle: the table as one side, an input as the other
    a, b = c.inputs[0], c.table
    want_rows = []
    for row in range(c.usable):
        na = int((a[:c.usable] == a[row]).all(axis=1).sum())
        nb = int((b[:c.usable] == a[row]).all(axis=1).sum())
        if na != nb:
            want_rows.append(row)
    assert H.shuffle_failures(a, b, c.usable) == want_rows
    assert H.shuffle_failures(a, a[::-1][c.n - c.usable:], c.usable) == []


def test_absent_values_are_absent_and_homed_where_asked():
    c = H.case("wrap")
    vals = H.absent_values(c, 5, home=62)
    present = set(H.keys_of(c.table[:c.usable]))
    assert len(set(H.keys_of(vals))) == 5 and not present & set(H.keys_of(vals))
    assert H.home_slots(vals, 64) == [62] * 5
    assert not set(H.keys_of(H.absent_values(H.case("padding"), 70))) & set(H.keys_of(H.case("padding").table))
