"""Adversarial inputs for the open-addressing hash tables of csrc/logup.hip and csrc/check.hip, with their references.
Pure Python and numpy: no GPU, no oracle.

The device tables probe linearly from key_hash(value) & (cap - 1) over the eight 32-bit limbs of the STORED (Montgomery) form.
Random field elements spread evenly over a table that is at most half full, so they never build a long probe chain, never wrap
past the last slot and rarely repeat.  Real tables are the Montgomery forms of small integers plus one padding value; the cases
below are built from exactly those keys, chosen by their home slot under the numpy twin of the device hash (which
tests/test_gpu_hash_tables.py pins to the device by reading a built slot table back).

  key_hash, table_capacity, home_slots, occupied_slots   the twins of logup.hpp::key_hash / logup_table_capacity and of a built table
  all_cases()                                            the cases: Case(name, table, inputs, usable, n, claim)
  multiplicities, lookup_failures, shuffle_failures      the references: dict / Counter, plain Python ints and lists
"""
from collections import Counter, namedtuple

import numpy as np

from h2util import R_MOD, to_mont

# `claim`: what the case's name promises, checked by tests/test_hash_table_cases_host.py under the twins alone
Case = namedtuple("Case", "name table inputs usable n claim")

SMALL = 1 << 16


# ---------------------------------------------------------------------------------------------- the twins
def key_hash(limbs):
    """logup.hpp::key_hash over (..., 8) uint32 limbs (least significant first) of the stored form; uint32 wrap-around"""
    limbs = np.asarray(limbs, dtype=np.uint32)
    assert limbs.shape[-1] == 8
    h = np.full(limbs.shape[:-1], 0x9E3779B9, dtype=np.uint32)
    with np.errstate(over="ignore"):
        for i in range(8):
            h = h ^ limbs[..., i]
            h = h * np.uint32(0x85EBCA6B)
            h = h ^ (h >> np.uint32(13))
        h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def limbs32(a):
    """(n, 4) uint64 -> (n, 8) uint32, least significant limb first"""
    a = np.ascontiguousarray(a, dtype="<u8").reshape(-1, 4)
    return a.view("<u4").reshape(-1, 8)


def table_capacity(usable):
    """logup_table_capacity: 64, doubled while < 2 * usable"""
    cap = 64
    while cap < 2 * usable:
        cap <<= 1
    return cap


def home_slots(a, cap):
    """the slot each (n, 4) value probes first in a table of `cap` slots, as Python ints"""
    return [int(h) & (cap - 1) for h in key_hash(limbs32(a))]


def keys_of(a):
    return [tuple(int(x) for x in r) for r in np.asarray(a).reshape(-1, 4)]


def occupied_slots(values, cap):
    """the slots a linear-probing table of `cap` slots holds after the DISTINCT values of `values` were inserted -- a set that
    does not depend on the order of insertion (which value sits in which slot of a cluster does)"""
    distinct = list(dict.fromkeys(keys_of(values)))
    taken = set()
    for h in home_slots(np.array(distinct, dtype=np.uint64).reshape(-1, 4), cap):
        while h in taken:
            h = (h + 1) & (cap - 1)
        taken.add(h)
    return taken


# ---------------------------------------------------------------------------------------------- the references
def multiplicities(table, inputs, usable, n, rows=None):
    """(m, misses): m[r] = how often the value of table row r < usable occurs among the rows [rows[0], min(rows[1], usable))
    (default: all usable rows) of every input, a duplicated table value credited to its FIRST row; rows >= usable get nothing;
    misses = input values absent from the usable table rows"""
    first = {}
    for i, key in enumerate(keys_of(table[:usable])):
        first.setdefault(key, i)
    lo, hi = (0, usable) if rows is None else (rows[0], min(rows[1], usable))
    m, misses = [0] * n, 0
    for a in inputs:
        for key in keys_of(a[lo:hi]) if lo < hi else []:
            r = first.get(key)
            if r is None:
                misses += 1
            else:
                m[r] += 1
    return m, misses


def lookup_failures(table, inputs, tags, usable, index=0):
    """per row < usable, the FIRST input in order whose value is absent from the usable table rows: (index, tag, row), sorted;
    `index` is the lookup's own"""
    present = set(keys_of(table[:usable]))
    ins = [keys_of(a[:usable]) for a in inputs]
    out = []
    for row in range(usable):
        for j, keys in enumerate(ins):
            if keys[row] not in present:
                out.append((int(index), int(tags[j]), row))
                break
    return sorted(out)


def shuffle_failures(input, shuffle, usable):
    """the input rows < usable whose value occurs a different number of times among the usable rows of the two sides"""
    a, b = keys_of(input[:usable]), keys_of(shuffle[:usable])
    ca, cb = Counter(a), Counter(b)
    return [row for row in range(usable) if ca[a[row]] != cb[a[row]]]


# ---------------------------------------------------------------------------------------------- the keys
_small = {}


def small_keys():
    """the Montgomery forms of 0 .. 65535 -- a 16-bit range table's keys -- as an (65536, 4) uint64 array"""
    if "a" not in _small:
        _small["a"] = to_mont(range(SMALL))
    return _small["a"]


def small_by_home(cap):
    """home slot -> the small integers homed there in a table of `cap` slots, ascending"""
    if cap not in _small:
        by = {}
        for v, h in enumerate(home_slots(small_keys(), cap)):
            by.setdefault(h, []).append(v)
        _small[cap] = by
    return _small[cap]


def mont(values):
    return to_mont([int(v) % R_MOD for v in values])


def one_limb_pairs():
    """[(limb, a, b)]: stored forms below r that differ in exactly one 32-bit limb, for every limb (the lowest, the highest and
    the middle ones), as (4,) uint64 pairs.  Limb 7 differs in a low bit, so that both stay below r."""
    base = mont([0x1234567])[0]
    out = []
    for limb in range(8):
        l = limbs32(base).copy()
        l[0, limb] ^= np.uint32(1 << (3 + limb))
        other = l.view("<u8").reshape(4).astype(np.uint64)
        v = sum(int(x) << (64 * i) for i, x in enumerate(other))
        assert v < R_MOD
        out.append((limb, base.copy(), other))
    return out


def _column(n, rows, fill):
    """(n, 4): `rows` first, `fill` after"""
    a = np.empty((n, 4), dtype=np.uint64)
    a[:len(rows)] = rows
    a[len(rows):] = fill
    return a


def _pick(table, usable, rng, count):
    return table[rng.integers(0, usable, size=count)]


# ---------------------------------------------------------------------------------------------- the cases
def _wrap_table():
    """32 distinct range-table keys that all probe slot 62 of 64 first; the rows past usable repeat row 0"""
    usable, n = 32, 64
    vals = small_by_home(64)[62]
    table = _column(n, small_keys()[vals[:usable]], small_keys()[vals[0]])
    absent = small_keys()[vals[usable]]                 # the 33rd key of that home slot: walks the whole cluster
    return table, usable, n, absent, vals


def case_wrap():
    table, usable, n, absent, _ = _wrap_table()
    rng = np.random.default_rng(62)
    # every key once (so also the one at the end of the chain, whichever it is), then uneven draws; rows past usable hold
    # an ABSENT value: they are not looked up
    ins = [_column(n, table[rng.permutation(usable)], absent), _column(n, _pick(table, usable, rng, usable), absent),
           _column(n, table[np.minimum(rng.integers(0, 40, size=usable), usable - 1)], absent)]
    claim = dict(cap=64, homes={62}, occupied=[62, 63] + list(range(30)), misses=0)
    return Case("wrap", table, ins, usable, n, claim)


def case_full_cluster_miss():
    table, usable, n, absent, _ = _wrap_table()
    rng = np.random.default_rng(63)
    col = _column(n, table[rng.permutation(usable)], absent)
    col[17] = absent
    claim = dict(cap=64, homes={62}, occupied=[62, 63] + list(range(30)), misses=1, absent_home=62)
    return Case("full_cluster_miss", table, [col, _column(n, _pick(table, usable, rng, usable), absent)], usable, n, claim)


def case_capacity_step():
    """usable = 33 is the first size with 128 slots; its 33 keys all probe slot 126 of 128 first"""
    usable, n = 33, 64
    vals = small_by_home(128)[126]
    table = _column(n, small_keys()[vals[:usable]], small_keys()[vals[1]])
    rng = np.random.default_rng(126)
    ins = [_column(n, table[rng.permutation(usable)], table[0]), _column(n, _pick(table, usable, rng, usable), table[0])]
    claim = dict(cap=128, homes={126}, occupied=[126, 127] + list(range(31)), misses=0)
    return Case("capacity_step", table, ins, usable, n, claim)


ADJACENT_FIRST, ADJACENT_HOMES, ADJACENT_EACH = 500, 16, 30


def case_adjacent_homes():
    """30 keys on each of the 16 home slots 500..515 of 1024, in shuffled row order: the clusters merge into slots 500..979;
    the last 32 usable rows repeat earlier keys far from their first row"""
    usable, n = 512, 1024
    by = small_by_home(1024)
    vals = [v for h in range(ADJACENT_FIRST, ADJACENT_FIRST + ADJACENT_HOMES) for v in by[h][:ADJACENT_EACH]]
    rng = np.random.default_rng(500)
    distinct = small_keys()[rng.permutation(vals)]
    rows = np.concatenate([distinct, distinct[rng.permutation(len(distinct))[:usable - len(distinct)]]])
    absent = small_keys()[by[ADJACENT_FIRST][ADJACENT_EACH]]
    table = _column(n, rows, rows[7])
    ins = [_column(n, table[rng.permutation(usable)], absent), _column(n, _pick(table, usable, rng, usable), absent),
           _column(n, _pick(table, 40, rng, usable), absent)]
    first, count = ADJACENT_FIRST, ADJACENT_HOMES * ADJACENT_EACH
    claim = dict(cap=1024, homes=set(range(first, first + ADJACENT_HOMES)), occupied=list(range(first, first + count)), misses=0)
    return Case("adjacent_homes", table, ins, usable, n, claim)


FAR_A, FAR_B = (5, 300, 301, 700, 1023), (255, 256)


def _far_duplicates(collide):
    """value A at rows 5, 300, 301, 700 and 1023, value B at rows 255 and 256 (workgroups of 256 rows: different workgroups,
    one adjacent pair, one pair across a workgroup boundary), and 150 more values at two far rows each: whichever row of a
    value reaches the table first, its credits belong to the lowest.  `collide`: distinct keys with A's and B's home slots in
    the rows between the duplicates."""
    usable, n = 1030, 2048
    cap = table_capacity(usable)
    by = small_by_home(cap)
    homes = [h for h in sorted(by) if len(by[h]) >= 4]
    bucket_a, bucket_b = by[homes[0]], by[homes[1]]
    a, b = bucket_a[0], bucket_b[0]
    rng = np.random.default_rng(1030 + collide)
    fixed = {r: a for r in FAR_A}
    fixed.update({r: b for r in FAR_B})
    if collide:
        fixed.update({150: bucket_a[1], 500: bucket_a[2], 3: bucket_a[3], 100: bucket_b[1], 254: bucket_b[2], 257: bucket_b[3]})
    used = set(bucket_a) | set(bucket_b)
    free = [r for r in rng.permutation(usable) if int(r) not in fixed]
    pool = [int(v) for v in rng.permutation(SMALL) if int(v) not in used]
    rows_of = dict(fixed)
    pairs = {}
    for i in range(150):                                    # two far rows each
        lo, hi = sorted((int(free[2 * i]), int(free[2 * i + 1])))
        rows_of[lo] = rows_of[hi] = pool[i]
        pairs[pool[i]] = (lo, hi)
    for j, r in enumerate(free[300:]):
        rows_of[int(r)] = pool[150 + j]
    vals = [rows_of[r] for r in range(usable)]
    table = _column(n, small_keys()[vals], small_keys()[a])
    absent = small_keys()[pool[-1]]
    hot = np.array([5, 300, 301, 700, 1023, 255, 256] * 8 + [hi for _, hi in pairs.values()])
    ins = [_column(n, table[rng.permutation(usable)], absent),
           _column(n, table[np.concatenate([hot, rng.integers(0, usable, size=usable - len(hot))])], absent)]
    claim = dict(cap=cap, misses=0, duplicates={a: FAR_A, b: FAR_B}, pairs=pairs,
                 colliders={a: bucket_a[1:4], b: bucket_b[1:4]} if collide else {})
    return Case("far_duplicates_collision" if collide else "far_duplicates", table, ins, usable, n, claim)


def case_far_duplicates():
    return _far_duplicates(0)


def case_far_duplicates_collision():
    return _far_duplicates(1)


HOT_COUNTS = [(1, 2, 3, 5), (5, 3, 2, 1), (3, 5, 1, 2), (2, 1, 5, 3)]
# lanes of a wave by the value they hold: shares of 1, 2, 3 and 5 distinct values, uneven
WAVE_SHARES = {1: [64], 2: [50, 14], 3: [40, 20, 4], 5: [30, 16, 9, 6, 3]}


def _wave(rng, table, usable, distinct):
    """64 rows holding exactly `distinct` table values in the shares above, the lanes interleaved"""
    picks = rng.choice(usable, size=distinct, replace=False)
    lanes = np.concatenate([np.full(s, p) for s, p in zip(WAVE_SHARES[distinct], picks)])
    return table[rng.permutation(lanes)]


def case_hot_waves():
    """usable = 250 of 256 rows: four waves per column, the last one partial.  Column j gives wave w the distinct-value
    count HOT_COUNTS[j][w]; a wave of one value has all 64 lanes hit one row."""
    usable, n = 250, 256
    rng = np.random.default_rng(250)
    vals = rng.permutation(SMALL)[:usable]
    table = _column(n, small_keys()[vals], small_keys()[vals[2]])
    ins = []
    for counts in HOT_COUNTS:
        col = np.concatenate([_wave(rng, table, usable, d) for d in counts])
        ins.append(col.copy())
    claim = dict(cap=512, misses=0, wave_counts=HOT_COUNTS)
    return Case("hot_waves", table, ins, usable, n, claim)


PADDING_DISTINCT = 40


def case_padding():
    """40 distinct values, then one padding value up to usable = 1000 of 1024 rows; the rows past usable hold a value that
    also occurs inside (row 3) in the table AND in the inputs: they are never credited and never looked up"""
    usable, n = 1000, 1024
    rng = np.random.default_rng(1000)
    vals = rng.permutation(SMALL)[:PADDING_DISTINCT + 2]
    pad, absent = small_keys()[0], small_keys()[vals[-1]]          # padding is the field's zero, as in a real table
    assert 0 not in vals
    rows = np.concatenate([small_keys()[vals[:PADDING_DISTINCT]], np.repeat(pad[None], usable - PADDING_DISTINCT, axis=0)])
    table = _column(n, rows, rows[3])
    ins = []
    for j in range(3):
        idx = np.where(rng.random(usable) < 0.85, PADDING_DISTINCT + rng.integers(0, 900, size=usable),
                       rng.integers(0, PADDING_DISTINCT, size=usable))
        ins.append(_column(n, table[idx], table[3]))
    claim = dict(cap=2048, misses=0, padding_first=PADDING_DISTINCT, absent=absent)
    return Case("padding", table, ins, usable, n, claim)


def _hand_keys():
    return mont([0, 1, R_MOD - 1])


def case_one_limb_pairs():
    """0, 1, r - 1 and both members of every one-limb pair in the table, each hit a different number of times"""
    usable, n = 24, 32
    pairs = one_limb_pairs()
    rows = np.concatenate([_hand_keys(), np.array([pairs[0][1]] + [b for _, _, b in pairs]), small_keys()[2:14]])
    assert len(rows) == usable
    table = _column(n, rows, rows[0])
    hits = np.concatenate([np.full(1 + r % 5, r) for r in range(usable)])      # row r: 1 + r mod 5 hits
    ins = [_column(n, table[hits[:usable]], rows[4]), _column(n, table[hits[usable:2 * usable]], rows[4]),
           _column(n, table[np.concatenate([hits[2 * usable:], np.arange(usable)])[:usable]], rows[4])]
    claim = dict(cap=64, misses=0, pairs=pairs)
    return Case("one_limb_pairs", table, ins, usable, n, claim)


def case_one_limb_pairs_absent():
    """only the FIRST member of the pairs is in the table; each input value that is a second member is a miss"""
    usable, n = 24, 32
    pairs = one_limb_pairs()
    others = np.array([b for _, _, b in pairs])
    rows = np.concatenate([_hand_keys(), pairs[0][1][None], small_keys()[2:22]])
    assert len(rows) == usable
    table = _column(n, rows, rows[0])
    ins = [_column(n, np.concatenate([others, rows[:usable - 8]]), others[0]),
           _column(n, np.concatenate([rows[:usable - 8], others[::-1]]), others[7])]
    claim = dict(cap=64, misses=16, pairs=pairs)
    return Case("one_limb_pairs_absent", table, ins, usable, n, claim)


BUILDERS = (case_wrap, case_full_cluster_miss, case_capacity_step, case_adjacent_homes, case_far_duplicates,
            case_far_duplicates_collision, case_hot_waves, case_padding, case_one_limb_pairs, case_one_limb_pairs_absent)
NAMES = tuple(b.__name__[len("case_"):] for b in BUILDERS)
_built = {}


def case(name):
    """the named case, built once; callers must not modify its arrays"""
    if name not in _built:
        _built[name] = BUILDERS[NAMES.index(name)]()
        assert _built[name].name == name
        for a in [_built[name].table] + _built[name].inputs:
            a.setflags(write=False)
    return _built[name]


def all_cases():
    return [case(name) for name in NAMES]


def absent_values(c, count, home=None):
    """`count` range-table keys that are NOT among the usable rows of the case's table (with `home`: that probe this slot of
    the case's table first), as an (count, 4) array"""
    present = set(keys_of(c.table[:c.usable]))
    cap = table_capacity(c.usable)
    vals = small_by_home(cap)[home] if home is not None else range(SMALL - 1, 0, -1)
    out = []
    for v in vals:
        if tuple(int(x) for x in small_keys()[v]) not in present:
            out.append(v)
            if len(out) == count:
                return small_keys()[out]
    raise AssertionError("absent_values: only %d of %d keys" % (len(out), count))
