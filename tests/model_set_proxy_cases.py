"""Cases of the fitted tabular proxies on SGD / ABC model sets (djb.model_set.fit_proxy / .proxy_tables / .evalp_is_proxy / .evalp_pdf_proxy):
the sampling step and the light sample of dj_sgd / dj_abc per hit, the material named by id.

Expected values never come from the product.  They come from the ORACLE, per material -- om = param_space_cases.oracle_model(O, kind, row),
tab = O.tabular(om, res, shadow) --:
    sampling       proxy_is_cases.compose(O, om, tab, None, u1, u2, o)                              -> (weight, i, pdf)
    light sample   fr = O.eval(om, i, o, None, "evalp"), pdf = O.eval(tab, i, o, None, "pdf"), then the plugins' guard: fr = pdf = +0
                   where i.z <= 0 || o.z <= 0 (a NaN z does not take it)                             -> (fr, pdf)
    tables         O.tabular_tables(tab)'s p22 / sigma / qf
selected by id (merl_set_cases.select), inactive hits +0 in every output, compared as bits with NaNs matched (same_bits), every unit and
every component.  The fits and the compositions are computed once per (kind, res, shadow) and shared (lru_cache), read-only.

Main set: model_set_cases.rows(kind), M = 6, res 90, shadow on; the refit: res 16, shadow off.  sgd row 5 (p = 1025) is the degenerate
row: the oracle fits it to n_qf = 2 with non-finite table entries, its proxy pdf is 0 for every sample and about half its samples have
i.z <= 0 -- the per-lane n_qf case and the IEEE division by a zero pdf.  alternating_ids() gives it a batch of its own: row 0 / row 5 / dead
on every hit.  The other eleven (kind, row) pairs are regular: assert_conditions() holds the oracle's values to that.

Grid-stride: one trip of the two kernels' grid is TRIP hits (GRID_CAP workgroups of BLOCK, djb_kernels_model_set_proxy.hip; the launch code
caps the grid with grid_capped(n, BLOCK, GRID_CAP)); the second-trip batch is TRIP + 4096 - 179 hits, a 4 096-hit block tiled."""
import ctypes as C
import functools

import numpy as np

import merl_set_cases
import model_set_cases
import param_space_cases
import proxy_is_cases
from dj_brdf_amd import _lib, djb
from hit_calls import CANARY

select, active, same_bits, inactive_values = merl_set_cases.select, merl_set_cases.active, merl_set_cases.same_bits, merl_set_cases.inactive_values
KINDS, M, N = model_set_cases.KINDS, model_set_cases.M, model_set_cases.N
rows = model_set_cases.rows
FITS = ((90, True), (16, False))            # (res, shadow): the main fit and the refit
DEGENERATE = ("sgd", 5)                     # p = 1025
HOST_N = 4_001
BLOCK, GRID_CAP = 256, 256 * 16             # djb_kernels_model_set_proxy.hip: BLOCK, GRID_CAP
TRIP = GRID_CAP * BLOCK                     # djb_internal.hpp: MODEL_SET_PROXY_TRIP
TRIP_N = TRIP + 4096 - 179
RAGGED = (1, 63, 64, 65, 255, 257, 1000)
BIG_M = 300                                 # above both LDS row budgets (101 sgd, 211 abc): rows in global memory by default
TAB_P22, TAB_SIGMA, TAB_QF = 0, 1, 3        # include/djb_hip.h: DJB_TAB_*
PROXY_MAX_ENTRIES = 1 << 27                 # include/djb_hip.h: DJB_MODEL_SET_PROXY_MAX_ENTRIES


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def oracle_fit(kind, m, res, shadow):
    """(the oracle's model of row m, its tabular(res, shadow)); kept alive for the session"""
    import oraclelib
    O = oraclelib.oracle()
    om = param_space_cases.oracle_model(O, kind, rows(kind)[m])
    return om, O.tabular(om, res, shadow)


@functools.lru_cache(maxsize=None)
def oracle_tables(kind, m, res, shadow):
    """{"p22", "sigma", "qf"} of the oracle's fit, read-only"""
    import oraclelib
    t = oraclelib.oracle().tabular_tables(oracle_fit(kind, m, res, shadow)[1])
    out = {k: np.ascontiguousarray(t[k], np.float32) for k in ("p22", "sigma", "qf")}
    _frozen(*out.values())
    return out


@functools.lru_cache(maxsize=None)
def sampler_inputs(n=N):
    return _frozen(*proxy_is_cases.sampler_inputs(n))          # (o, u1, u2)


def light_inputs(n=N):
    i, o = merl_set_cases.eval_inputs()
    return i[:n], o[:n]


def material_ids(n=N, m=M):
    return merl_set_cases.material_ids(n, m)[0]


@functools.lru_cache(maxsize=None)
def sample_per_material(kind, res, shadow, n=N):
    """compose() of every row on sampler_inputs(n): M tuples (weight [n, 3], i [n, 3], pdf [n])"""
    import oraclelib
    O = oraclelib.oracle()
    o, u1, u2 = sampler_inputs(n)
    per = tuple(proxy_is_cases.compose(O, *oracle_fit(kind, m, res, shadow), None, u1, u2, o) for m in range(M))
    for r in per:
        _frozen(*r)
    return per


def _light(kind, m, res, shadow, i, o):
    import oraclelib
    O = oraclelib.oracle()
    om, tab = oracle_fit(kind, m, res, shadow)
    fr = O.eval(om, i, o, None, "evalp").astype(np.float32)
    pdf = O.eval(tab, i, o, None, "pdf").astype(np.float32)
    guard = (i[:, 2] <= 0) | (o[:, 2] <= 0)                      # false for a NaN z
    fr[guard] = 0
    pdf[guard] = 0
    return _frozen(fr, pdf)


@functools.lru_cache(maxsize=None)
def light_per_material(kind, res, shadow, n=N):
    """M tuples (fr [n, 3], pdf [n]) on light_inputs(n)"""
    i, o = light_inputs(n)
    return tuple(_light(kind, m, res, shadow, i, o) for m in range(M))


def select_all(per, ids, m=M):
    """the selection of every output of per-material tuples"""
    return tuple(select([r[c] for r in per], ids, m) for c in range(len(per[0])))


def expected_sample(kind, res=90, shadow=True, n=N, ids=None):
    ids = material_ids(n) if ids is None else ids
    return select_all(sample_per_material(kind, res, shadow, n), ids)


def expected_light(kind, res=90, shadow=True, n=N, ids=None):
    ids = material_ids(n) if ids is None else ids
    return select_all(light_per_material(kind, res, shadow, n), ids)


def assert_same(tag, got, want, names=("weight", "i", "pdf")):
    """every output, every unit, every component: bits equal, NaNs matched as NaNs"""
    assert len(got) == len(want) == len(names), (tag, len(got), len(want))
    for name, g, w in zip(names, got, want):
        g = np.asarray(g, np.float32); w = np.asarray(w, np.float32)
        assert g.shape == w.shape, (tag, name, g.shape, w.shape)
        ok = same_bits(g, w)
        if not ok.all():
            bad = np.argwhere(~ok)
            k = tuple(bad[0])
            raise AssertionError(f"{tag}: {name} differs in {len(bad)} of {ok.size} values, first at {k}: got {g[k]!r} want {w[k]!r}")


def assert_light(tag, got, want):
    assert_same(tag, got, want, ("fr", "pdf"))


def assert_tables(tag, got, kind, m, res, shadow):
    """got: {"p22", "sigma", "qf"} of material m of a set -> the oracle's tables of row m % M, bits and lengths"""
    want = oracle_tables(kind, m % M, res, shadow)
    for name in ("p22", "sigma", "qf"):
        g = np.asarray(got[name], np.float32)
        assert g.shape == want[name].shape, (tag, name, g.shape, want[name].shape)
        assert same_bits(g, want[name]).all(), (tag, name, int((~same_bits(g, want[name])).sum()))
    assert len(want["p22"]) == len(want["sigma"]) == res


def assert_conditions(res=90, shadow=True, n=N):
    """what the module's docstring says of the oracle's values, on the inputs the tests use: sampler_inputs(n) and the N light-sample pairs"""
    for kind in KINDS:
        sp, lp = sample_per_material(kind, res, shadow, n), light_per_material(kind, res, shadow)
        for m in range(M):
            w, i, pdf = sp[m]
            fr, lpdf = lp[m]
            if (kind, m) == DEGENERATE:
                t = oracle_tables(kind, m, res, shadow)
                assert len(t["qf"]) == 2 and not all(np.isfinite(t[k]).all() for k in ("p22", "sigma", "qf")), {k: len(v) for k, v in t.items()}
                assert not pdf.view(np.uint32).any(), "the degenerate row's proxy pdf is +0 for every sample"
                side = float((i[:, 2] <= 0).mean())
                assert 0.3 < side < 0.7, side
                assert not np.isfinite(w[~(i[:, 2] <= 0)]).all()          # the IEEE division by a zero pdf: Inf or NaN weights
                continue
            assert len(oracle_tables(kind, m, res, shadow)["qf"]) > 2
            good = np.isfinite(w).all(1) & (w > 0).any(1)
            assert good.mean() >= 0.5, (kind, m, float(good.mean()))
            lit = (lpdf > 0) & (fr > 0).any(1)
            assert lit.mean() >= 0.9, (kind, m, float(lit.mean()))


def alternating_ids(n=4096):
    """row 0 / the degenerate row / dead, on every hit"""
    dead = inactive_values(M)
    k = np.arange(n)
    ids = np.where(k % 3 == 0, 0, np.where(k % 3 == 1, DEGENERATE[1], dead[(k // 3) % len(dead)])).astype(np.int32)
    ids.setflags(write=False)
    return ids


def alternating_case(n=4096):
    """(ids, (o, u1, u2), the sampling expectation, (i, o), the light-sample expectation) on the first n hits of the main inputs, sgd"""
    ids = alternating_ids(n)
    head = lambda per: [tuple(a[:n] for a in r) for r in per]
    return (ids, tuple(a[:n] for a in sampler_inputs()), select_all(head(sample_per_material("sgd", 90, True)), ids),
            tuple(a[:n] for a in light_inputs()), select_all(head(light_per_material("sgd", 90, True)), ids))


def wall_ids(kind):
    """model_set_cases.wall_block's id pattern: the id changes with every active hit, every third hit is dead"""
    return model_set_cases.wall_block(kind)[0]


@functools.lru_cache(maxsize=None)
def big_ids(n=N):
    """random ids over [0, BIG_M) with 3 % dead hits; BIG_M - 1 is among them"""
    rng = np.random.default_rng(300)
    ids = rng.integers(0, BIG_M, n).astype(np.int32)
    dead = rng.choice(n, int(round(merl_set_cases.INACTIVE_SHARE * n)), replace=False)
    ids[dead] = rng.choice(inactive_values(BIG_M), dead.size)
    ids[7] = BIG_M - 1
    ids[8] = 0
    ids.setflags(write=False)
    return ids


def fold(ids, m_big=BIG_M):
    """the ids of a set whose material m holds row m % M -> ids into the main set (dead stays dead)"""
    return np.where(active(ids, m_big), ids % M, -1).astype(np.int32)


def big_rows(kind):
    return np.ascontiguousarray(rows(kind)[np.arange(BIG_M) % M])


def tiled(a, n):
    reps = -(-n // len(a))
    return np.ascontiguousarray(np.concatenate([a] * reps)[:n])


# ------------------------------------------------------------------ refusals through the C ABI (host arrays): the status, the message, nothing written
INVALID = 1

def _views(n):
    d = np.tile(np.float32([[0.3, 0.1, 0.9]]), (n, 1))
    return d, djb._Vec(d)


def c_sample(ctx, s, n=4, out_w=True, out_i=True, out_pdf=True, u=True, material=True):
    lib = _lib.load()
    d, vd = _views(n)
    ids = np.zeros(n, np.int32); u1 = np.full(n, 0.5, np.float32)
    w, i, pdf = np.full((n, 3), CANARY), np.full((n, 3), CANARY), np.full(n, CANARY)
    vw, vi = djb._Vec(w), djb._Vec(i)
    st = lib.djb_model_set_evalp_is_proxy_batch(ctx._h if ctx else None, s._h if s else None, C.c_int64(n), C.c_void_p(ids.ctypes.data) if material else None,
                                                C.c_void_p(u1.ctypes.data) if u else None, C.c_void_p(u1.ctypes.data), C.byref(vd.view),
                                                C.byref(vw.view) if out_w else None, C.byref(vi.view) if out_i else None,
                                                C.c_void_p(pdf.ctypes.data) if out_pdf else None, C.c_int(_lib.MEM_HOST))
    return st, lib.djb_last_error().decode(errors="replace"), (w, i, pdf)


def c_light(ctx, s, n=4, out_fr=True, out_pdf=True, material=True):
    lib = _lib.load()
    d, vd = _views(n)
    ids = np.zeros(n, np.int32)
    fr, pdf = np.full((n, 3), CANARY), np.full(n, CANARY)
    vfr = djb._Vec(fr)
    st = lib.djb_model_set_evalp_pdf_proxy_batch(ctx._h if ctx else None, s._h if s else None, C.c_int64(n), C.c_void_p(ids.ctypes.data) if material else None,
                                                 C.byref(vd.view), C.byref(vd.view), C.byref(vfr.view) if out_fr else None,
                                                 C.c_void_p(pdf.ctypes.data) if out_pdf else None, C.c_int(_lib.MEM_HOST))
    return st, lib.djb_last_error().decode(errors="replace"), (fr, pdf)


def assert_refusals(ctx, fitted, other_ctx):
    """every refusal of the five entry points on `ctx`; `fitted`: a set of ctx with a proxy"""
    lib = _lib.load()
    untouched = lambda outs: all((a == CANARY).all() for a in outs)
    bare = djb.model_set.from_rows("abc", rows("abc"), ctx=ctx)
    try:
        for call in (c_sample, c_light):                                # a call before fit_proxy
            st, msg, outs = call(ctx, bare)
            assert st == INVALID and "no proxy" in msg and untouched(outs), (st, msg)
        cnt = C.c_int(-5)
        assert lib.djb_model_set_get_proxy(bare._h, 0, TAB_P22, None, C.byref(cnt)) == INVALID and cnt.value == -5
        st = lib.djb_model_set_fit_proxy(ctx._h, bare._h, 2, 1)         # the reference's message (dj_brdf.h:2218)
        assert st == INVALID and "Invalid Resolution" in lib.djb_last_error().decode() and bare.proxy_info() == (0, False)
        st = lib.djb_model_set_fit_proxy(other_ctx._h, bare._h, 16, 1)
        assert st == INVALID and bare.proxy_info() == (0, False)
        assert lib.djb_model_set_fit_proxy(ctx._h, None, 16, 1) == INVALID and lib.djb_model_set_proxy_info(None, None, None) == INVALID
    finally:
        bare.close()
    for kw in (dict(out_w=False), dict(out_i=False), dict(out_pdf=False), dict(u=False), dict(material=False)):
        st, msg, outs = c_sample(ctx, fitted, **kw)
        assert st == INVALID and "null" in msg and untouched(outs), (kw, st, msg)
    for kw in (dict(out_fr=False), dict(out_pdf=False), dict(material=False)):
        st, msg, outs = c_light(ctx, fitted, **kw)
        assert st == INVALID and "null" in msg and untouched(outs), (kw, st, msg)
    for call in (c_sample, c_light):                                    # a set of another context, a null set, a null context
        st, msg, outs = call(other_ctx, fitted)
        assert st == INVALID and ("another context" in msg or "different back ends" in msg) and untouched(outs), (st, msg)
        st, msg, outs = call(ctx, None)
        assert st == INVALID and "null model set" in msg and untouched(outs), (st, msg)
        st, msg, outs = call(None, fitted)
        assert st == INVALID and "null ctx" in msg and untouched(outs), (st, msg)
        st, msg, outs = call(ctx, fitted)
        assert st == 0 and not untouched(outs), msg
    buf = np.full(90, CANARY, np.float32)
    for m in (-1, M):                                           # material out of range in get_proxy
        cnt = C.c_int(-5)
        st = lib.djb_model_set_get_proxy(fitted._h, m, TAB_P22, C.c_void_p(buf.ctypes.data), C.byref(cnt))
        assert st == INVALID and "outside" in lib.djb_last_error().decode() and cnt.value == -5 and (buf == CANARY).all()
    for which in (2, 4, 7):                                           # cdf and the Fresnel spline are not kept
        cnt = C.c_int(-5)
        assert lib.djb_model_set_get_proxy(fitted._h, 0, which, C.c_void_p(buf.ctypes.data), C.byref(cnt)) == INVALID and cnt.value == -5 and (buf == CANARY).all()
    cnt = C.c_int(-5)                                                 # out == NULL queries the count
    assert lib.djb_model_set_get_proxy(fitted._h, 0, TAB_QF, None, C.byref(cnt)) == 0 and 2 < cnt.value <= 90
