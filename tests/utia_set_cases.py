"""Cases of UTIA material sets (djb.utia_set / djb_utia_set_*): hits on M resident UTIA tables, each naming its material by id.

Expected values never come from the product's own single-material call.  They come from the ORACLE -- O.utia(path), the tables written
to a temporary directory -- per material, selected by id (merl_set_cases.select):
    want[k] = oracle_result_for_material[material[k]][k]      (active:   0 <= material[k] < M)
    want[k] = +0.0f                                           (inactive: any other id)
compared as bits.

Materials: the smooth synthetic table, a uniformly drawn one (values from -5 to 120: a wrong record shows, negative samples are clamped)
and the smooth table with its two azimuth axes reversed (the same values at other records); together a wrong material shows.

Pairs: merl_set_cases.eval_inputs() -- N = 40 001 with below-horizon blocks, zero vectors and NaN components -- and the ids of
merl_set_cases.material_ids().  A pair with a non-finite component has no defined UTIA value (the reference indexes without a range
check: proxy_is_cases.undefined_weight): it is not handed to the oracle and not compared where its hit is active; the product must
return for it without fault, and an inactive hit is +0 whatever its directions hold.  At most 1 % of the pairs may be left out this
way (those inputs: 192 of 40 001).

Grid-line block (grid_block): 4 096 pairs whose directions sit on the table's grid lines -- polar angles 15 a degrees, azimuths 7.5 b
degrees -- taken exact or one float step to either side in each of z, x, y: a cell estimate next to a cell boundary, an angle next
to a rounding boundary -- the pairs tier 1 of the kernels declines by construction.  All finite and above the horizon (z is kept at
or below 1: acos of more has no value); every third id is inactive."""
import functools
import os
import tempfile

import numpy as np

import merl_set_cases
from dj_brdf_amd import djb, synth

material_ids, select, active = merl_set_cases.material_ids, merl_set_cases.select, merl_set_cases.active
assert_ids_cover_every_class, same_bits = merl_set_cases.assert_ids_cover_every_class, merl_set_cases.same_bits

M = 3
N = merl_set_cases.N
UNDEFINED_MAX_SHARE = 0.01
GRID_N = 4096


@functools.lru_cache(maxsize=None)
def tables():
    smooth = synth.utia_table_smooth()
    drawn = np.random.default_rng(11).uniform(-5, 120, 3 * 288 * 288)
    reversed_ = np.ascontiguousarray(smooth.reshape(3, 6, 48, 6, 48)[:, :, ::-1, :, ::-1]).reshape(-1)
    t = (smooth, drawn, reversed_)
    for a in t:
        a.setflags(write=False)
    return t


def product_members(ctx):
    return [djb.utia.from_table(t, ctx=ctx) for t in tables()]


@functools.lru_cache(maxsize=None)
def oracle_materials():
    import oraclelib
    O = oraclelib.oracle()
    out = []
    with tempfile.TemporaryDirectory(prefix="utia_set_") as d:          # the oracle reads a UTIA table from a file, once
        for k, t in enumerate(tables()):
            path = os.path.join(d, f"m{k}.bin")
            np.asarray(t, np.float64).tofile(path)
            out.append(O.utia(path))
    return tuple(out)


def defined(i, o):
    """the pairs that have a UTIA value: every component finite"""
    return np.isfinite(i).all(1) & np.isfinite(o).all(1)


@functools.lru_cache(maxsize=None)
def eval_inputs():
    i, o = merl_set_cases.eval_inputs()
    out = int((~defined(i, o)).sum())
    assert 0 < out <= UNDEFINED_MAX_SHARE * len(i) and (len(i), out) == (40_001, 192), (len(i), out)
    return i, o


def _per_material(op, i, o):
    """the oracle's eval / evalp of every material: M arrays [n, 3] (read-only); NaN where the pair has no defined value"""
    import oraclelib
    O = oraclelib.oracle()
    ok = defined(i, o)
    per = []
    for om in oracle_materials():
        a = np.full((len(i), 3), np.nan, np.float32)
        a[ok] = O.eval(om, i[ok], o[ok], None, op)
        a.setflags(write=False)
        per.append(a)
    return tuple(per)


@functools.lru_cache(maxsize=None)
def eval_per_material(op):
    return _per_material(op, *eval_inputs())


def compared(ids, i, o):
    """[n] mask of the hits whose result is compared: every inactive hit, and the active ones with a defined value"""
    return defined(i, o) | ~active(ids, M)


def expected_eval(op, ids=None):
    ids = material_ids()[0] if ids is None else ids
    return select(eval_per_material(op), ids)


def assert_eval(tag, got, want, mask):
    got = np.asarray(got, np.float32)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    ok = same_bits(got, want) | ~mask[:, None]
    assert ok.all(), f"{tag}: {int((~ok).sum())} of {ok.size} values differ, first at {tuple(np.argwhere(~ok)[0])}"


# ------------------------------------------------------------------ the grid-line block
@functools.lru_cache(maxsize=None)
def grid_block():
    """(ids [4096] int32, i, o [4096, 3] float32), read-only"""
    rng = np.random.default_rng(4096)

    def dirs():
        a = rng.integers(0, 6, GRID_N); b = rng.integers(0, 48, GRID_N)            # 15 a < 90: above the horizon
        t = np.deg2rad(15.0 * a); p = np.deg2rad(7.5 * b)
        d = np.stack([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)], 1).astype(np.float32)
        step = rng.integers(-1, 2, (GRID_N, 3))                                    # per component: one float step down, exact, one up
        d = np.where(step < 0, np.nextafter(d, np.float32(-np.inf)), np.where(step > 0, np.nextafter(d, np.float32(np.inf)), d)).astype(np.float32)
        d[:, 2] = np.minimum(d[:, 2], np.float32(1))
        return d
    i, o = dirs(), dirs()
    assert defined(i, o).all() and (i[:, 2] > 0).all() and (o[:, 2] > 0).all()
    ids = rng.integers(0, M, GRID_N).astype(np.int32)
    dead = merl_set_cases.inactive_values(M)
    ids[2::3] = dead[np.arange(len(ids[2::3])) % len(dead)]
    for a in (ids, i, o):
        a.setflags(write=False)
    return ids, i, o


@functools.lru_cache(maxsize=None)
def grid_per_material(op):
    _, i, o = grid_block()
    return _per_material(op, i, o)


@functools.lru_cache(maxsize=None)
def grid_expected(op):
    ids, _, _ = grid_block()
    want = select(grid_per_material(op), ids)
    want.setflags(write=False)
    return want
