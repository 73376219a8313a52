"""Cases of MERL material sets (djb.merl_set / djb_merl_set_*): hits on M resident MERL tables, each naming its material by id.

Expected values never come from the product's own single-material calls.  They come from the ORACLE, per material, selected by id:
    want[k] = oracle_result_for_material[material[k]][k]      (active:   0 <= material[k] < M)
    want[k] = +0.0f in every output                           (inactive: any other id)
compared as bits, NaNs matched as NaNs (proxy_is_cases.same_bits / assert_same).

Materials: three synthetic tables with visibly different content -- the analytic one, the hashed one (a wrong bin shows) and the
grazing one; together a wrong material shows.  Proxy parameters: isotropic(0.3), elliptic(0.2, 0.5, 0.7) and isotropic(4.5e-3), the
sharp lobe whose samples tier 1 of the MERL index declines.  Sampling inputs: proxy_is_cases.sampler_inputs(40 001).

Ids (material_ids): a block in which the id changes every hit, a run of 300 equal ids, a uniformly random bulk, and inactive ids drawn
from {-1, M, M + 1, 2^31 - 1, -2^31} sprinkled over the bulk.  The tests assert that each material and the inactive class get at
least 1 000 hits of the bulk; 2 % of 40 001 hits would be 800, so the inactive share is 3 %."""
import functools

import numpy as np

import proxy_is_cases
from dj_brdf_amd import djb, synth

same_bits, assert_same = proxy_is_cases.same_bits, proxy_is_cases.assert_same

M = 3
N = 40_001
TABLES = (synth.merl_table, synth.merl_table_hashed, synth.merl_table_grazing)
ORACLE_PARAMS = (("elliptic", 0.3, 0.3, 0.0), ("elliptic", 0.2, 0.5, 0.7), ("elliptic", 4.5e-3, 4.5e-3, 0.0))
ALTERNATING = (0, 512)          # [begin, end): the id changes every hit
RUN = (600, 900)                # 300 equal ids
INACTIVE_SHARE = 0.03
BULK_MIN = 1000


def product_params():
    P = djb.microfacet.params
    return [P.isotropic(0.3), P.elliptic(0.2, 0.5, 0.7), P.isotropic(4.5e-3)]


@functools.lru_cache(maxsize=None)
def tables():
    t = tuple(f() for f in TABLES)
    for a in t:
        a.setflags(write=False)
    return t


def product_members(ctx):
    return [djb.merl.from_table(t, ctx=ctx) for t in tables()]


@functools.lru_cache(maxsize=None)
def oracle_materials():
    import oraclelib
    O = oraclelib.oracle()
    return tuple(O.merl_from_table(t) for t in tables())


def inactive_values(m=M):
    return np.array([-1, m, m + 1, 2 ** 31 - 1, -2 ** 31], np.int64).astype(np.int32)


@functools.lru_cache(maxsize=None)
def material_ids(n=N, m=M):
    """int32 [n] (read-only) and the mask of the bulk (neither the alternating block nor the run)"""
    rng = np.random.default_rng(20240)
    ids = rng.integers(0, m, n).astype(np.int32)
    bulk = np.ones(n, bool)
    a0, a1 = ALTERNATING
    ids[a0:a1] = (np.arange(a1 - a0) % m)[: max(0, min(a1, n) - a0)]
    bulk[a0:a1] = False
    r0, r1 = RUN
    ids[r0:r1] = 1 % m
    bulk[r0:r1] = False
    where = np.flatnonzero(bulk)
    dead = rng.choice(where, int(round(INACTIVE_SHARE * n)), replace=False) if len(where) else where
    ids[dead] = rng.choice(inactive_values(m), dead.size)
    ids.setflags(write=False); bulk.setflags(write=False)
    return ids, bulk


def active(ids, m=M):
    return (ids >= 0) & (ids < m)


def assert_ids_cover_every_class(ids, bulk, m=M):
    """the condition on the inputs: each material and the inactive class get at least 1 000 hits of the bulk"""
    b = ids[bulk]
    counts = [int((b == k).sum()) for k in range(m)] + [int((~active(b, m)).sum())]
    assert min(counts) >= BULK_MIN, counts
    for v in inactive_values(m):
        assert (b == v).any(), int(v)


@functools.lru_cache(maxsize=None)
def eval_inputs(n=N):
    """(i, o) [n, 3]: random pairs with blocks of either direction below the horizon, NaN components and zero vectors"""
    i = synth.directions_aos(n, synth.SEED_I).copy(); o = synth.directions_aos(n, synth.SEED_O).copy()
    s, k = 2000, 600
    o[s:s + k, 2] *= -1
    i[s + k:s + 2 * k, 2] *= -1
    s += 2 * k
    o[s:s + 64, 0] = np.nan; i[s + 64:s + 128, 2] = np.nan; i[s + 128:s + 192, 1] = np.nan
    o[s + 192:s + 256] = 0.0; i[s + 256:s + 320] = 0.0
    i[s + 320:s + 384] = (0, 0, 1); o[s + 320:s + 384] = (0, 0, 1)            # h on the normal, d on the normal
    i.setflags(write=False); o.setflags(write=False)
    return i, o


def select(per_material, ids, m=M):
    """want[k] = per_material[ids[k]][k] for active hits, +0 otherwise; per_material: m arrays [n] or [n, c]"""
    want = np.zeros_like(per_material[0])
    for k in range(m):
        sel = ids == k
        want[sel] = per_material[k][sel]
    return want


@functools.lru_cache(maxsize=None)
def eval_per_material(op):
    """the oracle's eval / evalp of every material on eval_inputs(): M arrays [N, 3], computed once (read-only)"""
    import oraclelib
    O = oraclelib.oracle()
    i, o = eval_inputs()
    per = tuple(O.eval(om, i, o, None, op).astype(np.float32) for om in oracle_materials())
    for a in per:
        a.setflags(write=False)
    return per


@functools.lru_cache(maxsize=None)
def sample_per_material(proxy_kind, oracle_params=ORACLE_PARAMS):
    """proxy_is_cases.compose of every material with its own parameters on sampler_inputs(N): M tuples (weight, i, pdf)"""
    import oraclelib
    O = oraclelib.oracle()
    o, u1, u2 = sampler_inputs()
    oproxy = O.microfacet(proxy_kind)
    per = tuple(proxy_is_cases.compose(O, om, oproxy, op, u1, u2, o) for om, op in zip(oracle_materials(), oracle_params))
    for res in per:
        for a in res:
            a.setflags(write=False)
    return per


@functools.lru_cache(maxsize=None)
def sampler_inputs():
    o, u1, u2 = proxy_is_cases.sampler_inputs(N)
    for a in (o, u1, u2):
        a.setflags(write=False)
    return o, u1, u2


def expected_eval(op, ids=None):
    ids = material_ids()[0] if ids is None else ids
    return select(eval_per_material(op), ids)


def expected_sample(proxy_kind, ids=None, oracle_params=ORACLE_PARAMS):
    """(weight [N, 3], i [N, 3], pdf [N])"""
    ids = material_ids()[0] if ids is None else ids
    per = sample_per_material(proxy_kind, oracle_params)
    return tuple(select([res[c] for res in per], ids) for c in range(3))
