"""Cases of the two per-hit proxy steps on a scene (djb.scene.evalp_is_proxy / .evalp_pdf_proxy, djb_scene_evalp_is_proxy_batch /
djb_scene_evalp_pdf_proxy_batch): the sampling step and the light sample of hits that land on a MERL set, a UTIA set, an sgd and an abc
model set at once.

Expected values never come from the product.  They come from the ORACLE, per slot, selected by scene id as scene_cases.expected selects:
every hit is handed to the oracle objects of ITS slot's material --
    merl m       merl_set_cases.oracle_materials()[m], the lobe O.microfacet(proxy kind) with merl_set_cases.ORACLE_PARAMS[m]
    utia m       utia_set_cases.oracle_materials()[m], the same lobe with UTIA_PARAMS[m] -- three sets DIFFERENT from the MERL set's, so that
                 a kernel that reads the wrong parameter block shows
    sgd / abc m  model_set_proxy_cases.oracle_fit(kind, m, 90, True): the oracle's model of row m and its tabular(90, True), no params
-- through the definitions the single-material cases use: proxy_is_cases.compose for sampling (weight, i, pdf; weight = pdf = 0 where
i.z <= 0, applied last), and for the light sample the oracle's evalp and the proxy's pdf, both zeroed where i.z <= 0 || o.z <= 0 (a numpy
comparison: a NaN z does not zero).  An id outside the table or a slot without material: +0 in every output.  Compared as bits, NaNs
matched as NaNs.

Inputs, one set for all kinds (N = 40 001): sampling merl_set_cases.sampler_inputs(), the light sample merl_set_light_cases.inputs(); ids
merl_set_cases.material_ids(N, n_slots) -- the mix scene_cases asserts: 621 of 625 waves hold all four kinds, 1 200 dead hits.  Tables:
scene_cases.TABLE (18 slots) and TABLE2 (20: permuted, a slot without material, an alias).

A UTIA hit whose i or o has a non-finite component has no defined fr / weight (proxy_is_cases.undefined_weight: the reference indexes its
table without a range check); such a pair is not handed to the oracle's utia object.  Those values of ACTIVE utia hits, and only those,
are left out of the comparison -- their direction and pdf are compared -- at most 1 % of all hits (assert_input_conditions)."""
import ctypes as C
import functools

import numpy as np

import merl_set_cases
import merl_set_light_cases
import model_set_cases
import model_set_proxy_cases
import proxy_is_cases
import scene_cases
import utia_set_cases
from hit_calls import CANARY

same_bits = merl_set_cases.same_bits
N = scene_cases.N
KINDS, COUNTS, TABLE, TABLE2, N_SLOTS = scene_cases.KINDS, scene_cases.COUNTS, scene_cases.TABLE, scene_cases.TABLE2, scene_cases.N_SLOTS
kind_of_ids, table_without, base = scene_cases.kind_of_ids, scene_cases.table_without, scene_cases.base
PROXY_KINDS = ("ggx", "beckmann")
UTIA_PARAMS = (("elliptic", 0.25, 0.25, 0.0), ("elliptic", 0.35, 0.15, -0.4), ("elliptic", 0.1, 0.1, 0.0))
assert not set(UTIA_PARAMS) & set(merl_set_cases.ORACLE_PARAMS) and len(UTIA_PARAMS) == utia_set_cases.M
MODEL_FIT = model_set_proxy_cases.FITS[0]
assert MODEL_FIT == (90, True) and model_set_cases.N == N == 40_001
UNDEFINED_MAX_SHARE = 0.01
LIVE_MIN = 200                  # per kind: active hits with a finite pdf > 0; with a non-zero fr / weight
GUARD_MIN = 100                 # per kind: light-sample hits that take the guard
NAN_Z_MIN = 10                  # active light-sample hits with a NaN z
TRIP = 256 * 16 * 256           # djb_internal.hpp: SCENE_PROXY_TRIP -- GRID_CAP workgroups of 256, every per-kind kernel of djb_kernels_scene_proxy.hip
TRIP_N = TRIP + 4096 - 179


def utia_product_params():
    from dj_brdf_amd import djb
    P = djb.microfacet.params
    return [P.isotropic(0.25), P.elliptic(0.35, 0.15, -0.4), P.isotropic(0.1)]


def prepare_members(members):
    """what the two calls need of the member sets scene_cases' tests build: proxy parameters on merl and utia, the (90, True) fit on sgd and abc"""
    members["merl"].set_proxy_params(merl_set_cases.product_params())
    members["utia"].set_proxy_params(utia_product_params())
    for kind in model_set_cases.KINDS:
        members[kind].fit_proxy(*MODEL_FIT)


def material_ids(n_slots=N_SLOTS):
    return merl_set_cases.material_ids(N, n_slots)[0]


def sampler_inputs():
    return merl_set_cases.sampler_inputs()               # (o, u1, u2)


def light_inputs():
    return merl_set_light_cases.inputs()                 # (i, o)


def _finite(*vs):
    ok = np.ones(len(vs[0]), bool)
    for v in vs:
        ok &= np.isfinite(v).all(1)
    return ok


# ------------------------------------------------------------------ the oracle of one slot's material on the hits that name it
def _slot_sample(O, proxy_kind, slot, o, u1, u2):
    kind, m = slot
    if kind == "merl":
        return proxy_is_cases.compose(O, merl_set_cases.oracle_materials()[m], O.microfacet(proxy_kind), merl_set_cases.ORACLE_PARAMS[m], u1, u2, o)
    if kind == "utia":
        return proxy_is_cases.compose(O, utia_set_cases.oracle_materials()[m], O.microfacet(proxy_kind), UTIA_PARAMS[m], u1, u2, o,
                                      undefined=lambda i: ~_finite(i, o))
    om, tab = model_set_proxy_cases.oracle_fit(kind, m, *MODEL_FIT)
    return proxy_is_cases.compose(O, om, tab, None, u1, u2, o)


def _slot_light(O, proxy_kind, slot, i, o):
    kind, m = slot
    if kind == "merl":
        return merl_set_light_cases.oracle_pair(O, merl_set_cases.oracle_materials()[m], O.microfacet(proxy_kind), merl_set_cases.ORACLE_PARAMS[m], i, o)
    if kind == "utia":
        target, proxy, params, ok = utia_set_cases.oracle_materials()[m], O.microfacet(proxy_kind), UTIA_PARAMS[m], _finite(i, o)
    else:
        target, proxy = model_set_proxy_cases.oracle_fit(kind, m, *MODEL_FIT)
        params, ok = None, np.ones(len(i), bool)
    with np.errstate(all="ignore"):
        fr = np.full((len(i), 3), np.nan, np.float32)
        if ok.any():
            fr[ok] = O.eval(target, np.ascontiguousarray(i[ok]), np.ascontiguousarray(o[ok]), None, "evalp")
        pdf = np.array(O.eval(proxy, i, o, params, "pdf"), np.float32).reshape(-1)
    z = merl_set_light_cases.guarded(i, o)
    fr[z] = 0.0; pdf[z] = 0.0
    return fr, pdf


def _select(fn, n_out, ids, table, arrays):
    """want[k] = fn(slot of ids[k], hit k) for active hits, +0 otherwise; every hit goes to the oracle once, with its own slot's material"""
    import oraclelib
    O = oraclelib.oracle()
    ids = np.asarray(ids)
    n = len(ids)
    out = tuple(np.zeros((n, 3), np.float32) if c < n_out - 1 else np.zeros(n, np.float32) for c in range(n_out))
    for s, slot in enumerate(table):
        sel = np.flatnonzero(ids == s)
        if slot is None or not len(sel):
            continue
        res = fn(O, slot, *(np.ascontiguousarray(a[sel]) for a in arrays))
        for dst, src in zip(out, res):
            dst[sel] = src
    return out


def expected_sample_on(proxy_kind, ids, table, o, u1, u2):
    """(weight [n, 3], i [n, 3], pdf [n])"""
    return _select(lambda O, slot, o_, a, b: _slot_sample(O, proxy_kind, slot, o_, a, b), 3, ids, table, (o, u1, u2))


def expected_light_on(proxy_kind, ids, table, i, o):
    """(fr [n, 3], pdf [n])"""
    return _select(lambda O, slot, i_, o_: _slot_light(O, proxy_kind, slot, i_, o_), 2, ids, table, (i, o))


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def expected_sample(proxy_kind, table=TABLE):
    """on sampler_inputs() under material_ids(len(table)); computed once, read-only"""
    return _frozen(expected_sample_on(proxy_kind, material_ids(len(table)), table, *sampler_inputs()))


@functools.lru_cache(maxsize=None)
def expected_light(proxy_kind, table=TABLE):
    return _frozen(expected_light_on(proxy_kind, material_ids(len(table)), table, *light_inputs()))


def head(arrays, n):
    return tuple(a[:n] for a in arrays)


# ------------------------------------------------------------------ what is compared
def compared_sample(ids, table, want_i, o):
    """[n] mask of the hits whose WEIGHT is compared: all but the active utia hits with a non-finite sampled direction or o"""
    return ~((kind_of_ids(ids, table) == KINDS.index("utia")) & ~_finite(np.asarray(want_i, np.float32), o))


def compared_light(ids, table, i, o):
    """[n] mask of the hits whose FR is compared"""
    return ~((kind_of_ids(ids, table) == KINDS.index("utia")) & ~_finite(i, o))


def _assert(tag, names, got, want, mask):
    assert len(got) == len(want) == len(names), (tag, len(got), len(want))
    for c, (name, g, w) in enumerate(zip(names, got, want)):
        g = np.asarray(g, np.float32); w = np.asarray(w, np.float32)
        assert g.shape == w.shape, (tag, name, g.shape, w.shape)
        ok = same_bits(g, w)
        if c == 0 and mask is not None:
            ok |= ~mask[:, None]
        if not ok.all():
            bad = np.argwhere(~ok)
            k = tuple(bad[0])
            raise AssertionError(f"{tag}: {name} differs in {len(bad)} of {ok.size} values, first at {k}: got {g[k]!r} want {w[k]!r}")


def assert_sample(tag, got, want, mask=None):
    """(weight, i, pdf): bits equal, NaNs matched; mask: the hits whose weight is compared (direction and pdf always are)"""
    _assert(tag, ("weight", "i", "pdf"), got, want, mask)


def assert_light(tag, got, want, mask=None):
    _assert(tag, ("fr", "pdf"), got, want, mask)


def differs(got, want, mask):
    """does any compared value of the first output differ?"""
    return not (same_bits(np.asarray(got[0], np.float32), want[0]) | ~mask[:, None]).all()


def assert_input_conditions():
    """what the inputs must exercise, on oracle values only: the id mix, the cap on what is left out, and live / guarded / NaN hits of every kind"""
    ids = material_ids()
    scene_cases.assert_inputs_are_what_the_module_says()           # every slot hit, 621 of 625 waves with all four kinds, 1 200 dead hits
    kinds = kind_of_ids(ids)
    assert all((ids == s).sum() >= 2048 for s in range(N_SLOTS)) and int((kinds < 0).sum()) == 1200
    o, u1, u2 = sampler_inputs()
    li, lo = light_inputs()
    z = merl_set_light_cases.guarded(li, lo)
    nan_z = np.isnan(li[:, 2]) | np.isnan(lo[:, 2])
    assert int(((kinds >= 0) & nan_z).sum()) >= NAN_Z_MIN
    for pk in PROXY_KINDS:
        w, i, pdf = expected_sample(pk)
        fr, lpdf = expected_light(pk)
        left_s, left_l = ~compared_sample(ids, TABLE, i, o), ~compared_light(ids, TABLE, li, lo)
        assert 0 < left_s.sum() <= UNDEFINED_MAX_SHARE * N and 0 < left_l.sum() <= UNDEFINED_MAX_SHARE * N, (pk, int(left_s.sum()), int(left_l.sum()))
        assert not any(a[kinds < 0].view(np.uint32).any() for a in (w, i, pdf, fr, lpdf))
        for q, kind in enumerate(KINDS):
            sel = kinds == q
            live = lambda p, v, s: (int((np.isfinite(p[s]) & (p[s] > 0)).sum()), int((np.nan_to_num(v[s], posinf=1, neginf=1) != 0).any(1).sum()))
            assert min(live(pdf, w, sel)) >= LIVE_MIN, (pk, kind, "sampling", live(pdf, w, sel))
            assert min(live(lpdf, fr, sel & ~z)) >= LIVE_MIN, (pk, kind, "light", live(lpdf, fr, sel & ~z))
            assert int((sel & z).sum()) >= GUARD_MIN, (kind, int((sel & z).sum()))
            assert not fr[sel & z].view(np.uint32).any() and not lpdf[sel & z].view(np.uint32).any()


# ------------------------------------------------------------------ second tiers inside a mixed batch
BLOCK_N = scene_cases.BLOCK_N


def _interleave(kind, local_ids, block_arrays, main_arrays):
    """even positions: the block of `kind` (its inactive hits stay inactive); odd positions: the first BLOCK_N hits of the main batch, those of
    `kind` moved to another kind (scene_cases.mixed_block's construction)"""
    assert len(local_ids) == BLOCK_N
    sid = np.where(merl_set_cases.active(local_ids, COUNTS[kind]), local_ids + base(kind), -1).astype(np.int32)
    mids = np.array(material_ids()[:BLOCK_N])
    same = kind_of_ids(mids) == KINDS.index(kind)
    mids[same] += scene_cases.NEXT_KIND[kind]
    if kind == "abc":
        mids[same] %= 3
    assert not (kind_of_ids(mids) == KINDS.index(kind)).any() and (kind_of_ids(mids) >= 0).sum() > BLOCK_N // 2
    ids = np.empty(2 * BLOCK_N, np.int32)
    ids[0::2], ids[1::2] = sid, mids
    out = []
    for b, m in zip(block_arrays, main_arrays):
        a = np.empty((2 * BLOCK_N,) + b.shape[1:], np.float32)
        a[0::2], a[1::2] = b, m[:BLOCK_N]
        out.append(a)
    return _frozen((ids,) + tuple(out))


@functools.lru_cache(maxsize=None)
def mixed_light(kind):
    """(ids, i, o) [8192]: merl -- merl_set_light_cases.declined_block(), the pairs tier 1 of the MERL index declines; sgd / abc -- the wall block"""
    lids, bi, bo = merl_set_light_cases.declined_block(BLOCK_N) if kind == "merl" else model_set_cases.wall_block(kind)
    return _interleave(kind, lids, (bi, bo), light_inputs())


@functools.lru_cache(maxsize=None)
def mixed_sample(kind):
    """(ids, o, u1, u2) [8192]: the block's id pattern and its o on the even positions with the main batch's uniforms.  merl: o next to the
    normal under the sharp third lobe -- the samples tier 1 declines; sgd / abc: the wall block's ids, a new row on every active hit"""
    lids, _, bo = merl_set_light_cases.declined_block(BLOCK_N) if kind == "merl" else model_set_cases.wall_block(kind)
    o, u1, u2 = sampler_inputs()
    return _interleave(kind, lids, (bo, u1[BLOCK_N:2 * BLOCK_N], u2[BLOCK_N:2 * BLOCK_N]), (o, u1, u2))


@functools.lru_cache(maxsize=None)
def mixed_light_expected(proxy_kind, kind):
    ids, i, o = mixed_light(kind)
    return _frozen(expected_light_on(proxy_kind, ids, TABLE, i, o))


@functools.lru_cache(maxsize=None)
def mixed_sample_expected(proxy_kind, kind):
    ids, o, u1, u2 = mixed_sample(kind)
    return _frozen(expected_sample_on(proxy_kind, ids, TABLE, o, u1, u2))


def tiled(head_arrays, block_arrays, n):
    """the head, then the block repeated up to n units in all"""
    out = []
    for h, b in zip(head_arrays, block_arrays):
        reps = -(-(n - len(h)) // len(b))
        out.append(np.ascontiguousarray(np.concatenate([h] + [b] * reps)[:n]))
    return tuple(out)


# ------------------------------------------------------------------ the C ABI's refusals (host arrays): the status, the message, nothing written
INVALID, NOT_IMPLEMENTED = 1, 5


def c_sample(ctx, s, proxy, n=4, out_pdf=True, out_w=True, material=True):
    from dj_brdf_amd import _lib, djb
    lib = _lib.load()
    d = np.tile(np.float32([[0.3, 0.1, 0.9]]), (n, 1)); vd = djb._Vec(d)
    ids = np.zeros(n, np.int32); u = np.full(n, 0.5, np.float32)
    w, i, pdf = np.full((n, 3), CANARY), np.full((n, 3), CANARY), np.full(n, CANARY)
    vw, vi = djb._Vec(w), djb._Vec(i)
    st = lib.djb_scene_evalp_is_proxy_batch(ctx._h if ctx else None, s._h if s else None, proxy._h if proxy else None, C.c_int64(n),
                                            C.c_void_p(ids.ctypes.data) if material else None, C.c_void_p(u.ctypes.data), C.c_void_p(u.ctypes.data),
                                            C.byref(vd.view), C.byref(vw.view) if out_w else None, C.byref(vi.view),
                                            C.c_void_p(pdf.ctypes.data) if out_pdf else None, C.c_int(_lib.MEM_HOST))
    return st, lib.djb_last_error().decode(errors="replace"), (w, i, pdf)


def c_light(ctx, s, proxy, n=4, out_pdf=True, out_w=True, material=True):
    from dj_brdf_amd import _lib, djb
    lib = _lib.load()
    d = np.tile(np.float32([[0.3, 0.1, 0.9]]), (n, 1)); vd = djb._Vec(d)
    ids = np.zeros(n, np.int32)
    fr, pdf = np.full((n, 3), CANARY), np.full(n, CANARY)
    vfr = djb._Vec(fr)
    st = lib.djb_scene_evalp_pdf_proxy_batch(ctx._h if ctx else None, s._h if s else None, proxy._h if proxy else None, C.c_int64(n),
                                             C.c_void_p(ids.ctypes.data) if material else None, C.byref(vd.view), C.byref(vd.view),
                                             C.byref(vfr.view) if out_w else None, C.c_void_p(pdf.ctypes.data) if out_pdf else None, C.c_int(_lib.MEM_HOST))
    return st, lib.djb_last_error().decode(errors="replace"), (fr, pdf)


def assert_refusals(ctx, main, members, lobes, other_ctx, other_lobe, build_members):
    """every refusal of the two entry points on `ctx`; build_members(prepared=False): fresh member sets of ctx without parameters or fits"""
    from dj_brdf_amd import djb
    untouched = lambda outs: all((a == CANARY).all() for a in outs)
    for call in (c_sample, c_light):
        st, msg, outs = call(ctx, main, None)                                         # NULL proxy on a scene with merl / utia members
        assert st == INVALID and "null brdf (proxy)" in msg and untouched(outs), (st, msg)
        wrong = djb.tabular(djb.ggx(ctx=ctx), 16, True, ctx=ctx)
        st, msg, outs = call(ctx, main, wrong)                                        # another proxy kind
        assert st == NOT_IMPLEMENTED and "ggx or beckmann" in msg and untouched(outs), (st, msg)
        wrong.close()
        st, msg, outs = call(ctx, main, other_lobe)                                   # a lobe of another context
        assert st == INVALID and untouched(outs), (st, msg)
        st, msg, outs = call(other_ctx, main, lobes["ggx"])                           # a scene of another context
        assert st == INVALID and ("another context" in msg or "different back ends" in msg) and untouched(outs), (st, msg)
        st, msg, outs = call(ctx, None, lobes["ggx"])
        assert st == INVALID and "null scene" in msg and untouched(outs), (st, msg)
        st, msg, outs = call(None, main, lobes["ggx"])
        assert st == INVALID and "null ctx" in msg and untouched(outs), (st, msg)
        for kw in (dict(out_pdf=False), dict(out_w=False), dict(material=False)):
            st, msg, outs = call(ctx, main, lobes["ggx"], **kw)
            assert st == INVALID and "null" in msg and untouched(outs), (kw, st, msg)
        st, msg, outs = call(ctx, main, lobes["ggx"])
        assert st == 0 and not untouched(outs), msg
    bare = build_members(ctx, prepared=False)
    try:
        for kind, needle in (("merl", "merl member has no proxy parameters"), ("utia", "utia member has no proxy parameters"),
                             ("sgd", "sgd member has no proxy"), ("abc", "abc member has no proxy")):
            s = djb.scene(slots=[(kind, 0)], ctx=ctx, **{kind: bare[kind]})
            for call in (c_sample, c_light):
                st, msg, outs = call(ctx, s, lobes["ggx"])
                assert st == INVALID and needle in msg and untouched(outs), (kind, st, msg)
            s.close()
        s = djb.scene(slots=[("abc", 0)], ctx=ctx, abc=members["abc"])                 # model members alone: no lobe needed, any lobe ignored
        for call in (c_sample, c_light):
            for lobe in (None, lobes["ggx"], other_lobe):
                st, msg, outs = call(ctx, s, lobe)
                assert st == 0 and not untouched(outs), (st, msg)
        s.close()
    finally:
        for m in bare.values():
            m.close()
