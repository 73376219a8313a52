"""Cases of scenes (djb.scene / djb_scene_*): hits that land on a MERL set, a UTIA set, an sgd and an abc model set at once, each naming its
material by SCENE id through the scene's slot table.

Expected values never come from the product's own set calls.  They come from the ORACLE, per material, exactly as the three set case
modules take them, concatenated in slot order and selected by scene id (merl_set_cases.select):
    want[k] = oracle_result_for_slot[material[k]][k]      (active:   0 <= material[k] < n_slots, the slot has a material)
    want[k] = +0.0f                                       (inactive: any other id, or a slot without material)
compared as bits, NaNs matched as NaNs.

The main scene has 18 slots: 0-2 the MERL members of merl_set_cases, 3-5 the UTIA members of utia_set_cases, 6-11 the six sgd rows and
12-17 the six abc rows of model_set_cases.  Pairs: merl_set_cases.eval_inputs() (N = 40 001, what all four modules use); ids:
merl_set_cases.material_ids(N, 18).  A UTIA hit with a non-finite component has no defined value (utia_set_cases.defined): ACTIVE UTIA hits
of that kind, and only those, are left out of the comparison -- at most 1 % of all hits (the inputs have 192 non-finite pairs, about a
sixth of which land on UTIA slots).

The second table (TABLE2) holds the same members in permuted slot order, one slot without material and one alias -- two slots on one
material -- over 20 slots: a result that ignores the table shows.

Mixed blocks (mixed_block): each kind's second-tier block -- utia_set_cases.grid_block(), model_set_cases.wall_block(kind) -- on the even
positions, hits of the OTHER kinds (the first 4 096 pairs of the main batch) on the odd ones."""
import functools

import numpy as np

import merl_set_cases
import model_set_cases
import utia_set_cases

select, same_bits = merl_set_cases.select, merl_set_cases.same_bits
N = merl_set_cases.N
KINDS = ("merl", "utia", "sgd", "abc")
COUNTS = {"merl": merl_set_cases.M, "utia": utia_set_cases.M, "sgd": model_set_cases.M, "abc": model_set_cases.M}
NONE = None                                                      # a slot without material (djb.scene takes None)
TABLE = tuple((kind, m) for kind in KINDS for m in range(COUNTS[kind]))
N_SLOTS = len(TABLE)
assert N_SLOTS == 18 and TABLE[3] == ("utia", 0) and TABLE[6] == ("sgd", 0) and TABLE[12] == ("abc", 0)
UNDEFINED_MAX_SHARE = 0.01
SCENE_MAX_SLOTS = 1 << 20                                        # include/djb_hip.h: DJB_SCENE_MAX_SLOTS


def _table2():
    perm = np.random.default_rng(18).permutation(N_SLOTS)
    t = [TABLE[p] for p in perm]
    t.insert(7, NONE)
    t.append(("merl", 1))                                        # an alias: the second slot on this material
    return tuple(t)


TABLE2 = _table2()
assert len(TABLE2) == 20 and TABLE2.count(("merl", 1)) == 2 and TABLE2.count(NONE) == 1 and TABLE2[:N_SLOTS] != TABLE


def base(kind):
    """the first slot of `kind` in TABLE"""
    return TABLE.index((kind, 0))


def kind_of_ids(ids, table=TABLE):
    """[n] index into KINDS, -1 for an inactive hit"""
    code = np.array([-1 if s is None else KINDS.index(s[0]) for s in table], np.int64)
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < len(table))
    return np.where(ok, code[np.where(ok, ids, 0)], -1)


def eval_inputs():
    return merl_set_cases.eval_inputs()


def material_ids(n_slots=N_SLOTS):
    return merl_set_cases.material_ids(N, n_slots)


def assert_inputs_are_what_the_module_says():
    """the conditions on the ids: every slot and the inactive class are covered, and waves mix all four kinds"""
    ids, bulk = material_ids()
    merl_set_cases.assert_ids_cover_every_class(ids, bulk, N_SLOTS)
    per_slot = [int((ids[bulk] == s).sum()) for s in range(N_SLOTS)]
    assert 2048 <= min(per_slot) and max(per_slot) <= 2210, per_slot
    kinds = kind_of_ids(ids)
    assert int((kinds < 0).sum()) == 1200
    waves = kinds[: (N // 64) * 64].reshape(-1, 64)
    full = sum(all((w == q).any() for q in range(4)) for w in waves)
    assert (len(waves), full) == (625, 621), (len(waves), full)
    i, o = eval_inputs()
    left_out = ~compared(ids, i, o)
    assert 0 < left_out.sum() <= UNDEFINED_MAX_SHARE * N, int(left_out.sum())
    assert int((~utia_set_cases.defined(i, o)).sum()) == 192 and 16 <= left_out.sum() <= 64, int(left_out.sum())


def compared(ids, i, o, table=TABLE):
    """[n] mask of the hits whose result is compared: all but the ACTIVE UTIA hits without a defined value"""
    return ~((kind_of_ids(ids, table) == KINDS.index("utia")) & ~utia_set_cases.defined(i, o))


def _per_kind(kind, op):
    if kind == "merl":
        return merl_set_cases.eval_per_material(op)
    if kind == "utia":
        return utia_set_cases.eval_per_material(op)
    return model_set_cases.eval_per_material(kind, op)


@functools.lru_cache(maxsize=None)
def per_slot(op, table=TABLE):
    """the oracle's eval / evalp of every slot's material on eval_inputs(): len(table) arrays [N, 3] (shared, read-only)"""
    zero = np.zeros((N, 3), np.float32)
    zero.setflags(write=False)
    return tuple(zero if s is None else _per_kind(s[0], op)[s[1]] for s in table)


def expected(op, ids=None, table=TABLE, n=N):
    """want [n, 3] of the first n pairs of eval_inputs() under `ids`"""
    ids = material_ids(len(table))[0] if ids is None else ids
    return select([a[:n] for a in per_slot(op, table)], np.asarray(ids)[:n], len(table))


def table_without(kinds_absent, table=TABLE):
    """`table` with every slot of an absent kind turned into a slot without material"""
    return tuple(NONE if s is None or s[0] in kinds_absent else s for s in table)


def assert_eval(tag, got, want, mask=None):
    got = np.asarray(got, np.float32)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    ok = same_bits(got, want)
    if mask is not None:
        ok |= ~mask[:, None]
    assert ok.all(), (f"{tag}: {int((~ok).sum())} of {ok.size} values differ, first at {tuple(np.argwhere(~ok)[0])}: "
                      f"got {got[tuple(np.argwhere(~ok)[0])]!r} want {want[tuple(np.argwhere(~ok)[0])]!r}")


# ------------------------------------------------------------------ each kind's second-tier block inside a mixed batch
BLOCK_N = 4096
NEXT_KIND = {"merl": 3, "utia": 3, "sgd": 6, "abc": -12}             # slot shift that moves a hit of the block's kind onto another kind


def _block(kind):
    if kind == "utia":
        return utia_set_cases.grid_block()
    return model_set_cases.wall_block(kind)


def _block_expected(kind, op):
    return utia_set_cases.grid_expected(op) if kind == "utia" else model_set_cases.wall_expected(kind, op)


@functools.lru_cache(maxsize=None)
def mixed_block(kind):
    """(scene ids [8192] int32, i, o [8192, 3], mask [8192]), read-only: even positions the block of `kind` (its inactive hits stay
    inactive), odd positions the first 4 096 hits of the main batch, those of `kind` moved to another kind"""
    lids, bi, bo = _block(kind)
    assert len(lids) == BLOCK_N
    sid = np.where(merl_set_cases.active(lids, COUNTS[kind]), lids + base(kind), -1).astype(np.int32)
    mids = np.array(material_ids()[0][:BLOCK_N])
    same = kind_of_ids(mids) == KINDS.index(kind)
    mids[same] += NEXT_KIND[kind]
    if kind == "abc":
        mids[same] %= 3
    assert not (kind_of_ids(mids) == KINDS.index(kind)).any() and (kind_of_ids(mids) >= 0).sum() > BLOCK_N // 2
    mi, mo = (a[:BLOCK_N] for a in eval_inputs())
    ids = np.empty(2 * BLOCK_N, np.int32); i = np.empty((2 * BLOCK_N, 3), np.float32); o = np.empty_like(i)
    ids[0::2], ids[1::2] = sid, mids
    i[0::2], i[1::2] = bi, mi
    o[0::2], o[1::2] = bo, mo
    mask = compared(ids, i, o)
    for a in (ids, i, o, mask):
        a.setflags(write=False)
    return ids, i, o, mask


@functools.lru_cache(maxsize=None)
def mixed_expected(kind, op):
    ids = mixed_block(kind)[0]
    want = np.empty((2 * BLOCK_N, 3), np.float32)
    want[0::2] = _block_expected(kind, op)
    want[1::2] = expected(op, ids[1::2], n=BLOCK_N)
    want.setflags(write=False)
    return want
