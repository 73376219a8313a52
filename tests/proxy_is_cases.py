"""Cases of proxy importance sampling (brdf.evalp_is_proxy / djb_evalp_is_proxy_batch): the per-bounce step of the dj_merl / dj_utia /
dj_sgd / dj_abc plugins -- direction and pdf from a fitted lobe (the proxy), f_r cos from the measured or data-driven BRDF (the target).

The expected values are the operator's definition written in numpy float32 over the ORACLE's separate operators:
    i      = oracle.sample(proxy, u1, u2, o, proxy_params)
    pdf    = oracle.eval(proxy, i, o, proxy_params, "pdf")
    weight = (float32(1) / pdf) * oracle.eval(target, i, o, None, "evalp")          per channel
    weight = 0, pdf = 0 where i.z <= 0                                              applied last; a NaN i.z does not take it
They are never taken from the product's own three calls.  Objects are synthetic only."""
import functools
import os
import tempfile

import numpy as np

from dj_brdf_amd import djb, synth

TARGETS = ("merl", "utia", "sgd", "abc")
# name -> (kind, oracle params); the product's params come from product_params()
PROXIES = {
    "ggx_iso": ("ggx", ("elliptic", 0.3, 0.3, 0.0)),
    "ggx_ell": ("ggx", ("elliptic", 0.2, 0.5, 0.7)),
    "beckmann_iso": ("beckmann", ("elliptic", 0.3, 0.3, 0.0)),
    "beckmann_ell": ("beckmann", ("elliptic", 0.2, 0.5, 0.7)),
    "tabular": ("tabular", None),                      # tabular(abc, 90)
    "tabular_aniso": ("tabular_aniso", None),          # tabular_anisotropic(utia, 12, 24)
}
# the 16 pairs of kinds the GPU kernels serve: every target with every proxy KIND; the second parameter set of the two analytic lobes
# rides along on alternating targets, so that both isotropic and elliptic parameters meet both kinds
GPU_PAIRS = [(t, p) for t in TARGETS for p in ("ggx_iso", "beckmann_ell", "tabular", "tabular_aniso")] + \
            [("merl", "ggx_ell"), ("abc", "ggx_ell"), ("utia", "beckmann_iso"), ("sgd", "beckmann_iso")]
MATERIAL = "gold-metallic-paint"


def product_params(proxy):
    op = PROXIES[proxy][1]
    if op is None:
        return None
    return djb.microfacet.params.isotropic(op[1]) if op[1] == op[2] and op[3] == 0.0 else djb.microfacet.params.elliptic(*op[1:])


def product_target(name, ctx):
    if name == "merl":
        return djb.merl.from_table(synth.merl_table_hashed(), ctx=ctx)
    if name == "utia":
        return djb.utia.from_table(synth.utia_table_smooth(), ctx=ctx)
    if name == "lambert":
        return djb.lambert(ctx=ctx)
    return getattr(djb, name)(MATERIAL, ctx=ctx)


def product_proxy(name, ctx):
    kind = PROXIES[name][0] if name in PROXIES else name
    if kind == "tabular":
        return djb.tabular(djb.abc(MATERIAL, ctx=ctx), 90, True, ctx=ctx)
    if kind == "tabular_aniso":
        return djb.tabular_anisotropic(product_target("utia", ctx), 12, 24, True, ctx=ctx)
    if kind == "lambert":
        return djb.lambert(ctx=ctx)
    return getattr(djb, kind)(ctx=ctx)


_tmp = None


@functools.lru_cache(maxsize=None)
def oracle_target(name):
    import oraclelib
    O = oraclelib.oracle()
    if name == "merl":
        return O.merl_from_table(synth.merl_table_hashed())
    if name == "utia":                                 # the oracle reads a UTIA table from a file
        global _tmp
        _tmp = _tmp or tempfile.TemporaryDirectory(prefix="proxy_is_")
        path = os.path.join(_tmp.name, "smooth_utia.bin")
        synth.utia_table_smooth().astype(np.float64).tofile(path)
        return O.utia(path)
    if name == "lambert":
        return O.lambert()
    return getattr(O, name)(MATERIAL)


@functools.lru_cache(maxsize=None)
def oracle_proxy(name):
    import oraclelib
    O = oraclelib.oracle()
    kind = PROXIES[name][0] if name in PROXIES else name
    if kind == "tabular":
        return O.tabular(O.abc(MATERIAL), 90, True)
    if kind == "tabular_aniso":
        return O.tabular_anisotropic(oracle_target("utia"), 12, 24, True)
    if kind == "lambert":
        return O.lambert()
    return O.microfacet(kind)


def sampler_inputs(n_bulk=150_001):
    """(o, u1, u2): a random bulk with the inputs that leave the common paths of the samplers mixed in -- uniforms at and next to the
    ends of [0, 1], o on the normal, within 1e-3 rad of it, grazing, on and below the horizon, zero, NaN.  The mix of
    tests/test_gpu_parity.py (_beckmann_sampler_cases), its block sizes in proportion to n_bulk."""
    rng = np.random.default_rng(77)
    o = synth.directions_aos(n_bulk, synth.SEED_O).copy()
    u1 = synth.uniforms(n_bulk, synth.SEED_U1).copy(); u2 = synth.uniforms(n_bulk, synth.SEED_U2).copy()
    k = rng.permutation(n_bulk)
    f = n_bulk / 150_001

    def take(m):
        nonlocal k
        m = max(1, int(round(m * f)))
        sel, k = k[:m], k[m:]
        return sel
    edge = np.array([0.0, 1e-7, 1e-6, 1e-5, 1e-3, 0.5, 1 - 1e-3, 1 - 1e-5, 1 - 1e-6, 1 - 6e-8, 1.0], np.float32)
    s = take(4000); u2[s] = rng.choice(edge, s.size)
    s = take(4000); u2[s] = np.float32(1) - rng.random(s.size, dtype=np.float32) * np.float32(4e-3)
    s = take(4000); u1[s] = rng.choice(edge, s.size)
    s = take(4000); u1[s] = rng.random(s.size, dtype=np.float32) * np.float32(1e-4)
    s = take(4000); u1[s] = np.float32(1) - rng.random(s.size, dtype=np.float32) * np.float32(1e-4)
    s = take(3000); o[s] = (0, 0, 1)
    s = take(3000); t = rng.random(s.size) * 1e-3; ph = rng.random(s.size) * 6.2831853
    o[s] = np.stack([np.sin(t) * np.cos(ph), np.sin(t) * np.sin(ph), np.cos(t)], 1).astype(np.float32)
    s = take(3000); z = (rng.random(s.size) * 2e-3).astype(np.float32); ph = rng.random(s.size) * 6.2831853
    o[s] = np.stack([np.sqrt(1 - z * z) * np.cos(ph), np.sqrt(1 - z * z) * np.sin(ph), z], 1).astype(np.float32)
    s = take(1000); o[s, 2] = -np.abs(o[s, 2])
    s = take(200); o[s, 0] = np.nan
    s = take(200); u1[s] = np.nan
    s = take(200); u2[s] = np.nan
    s = take(200); o[s] = 0.0
    return o, u1, u2


def undefined_weight(target, i, o):
    """utia::eval turns its angles into table indices without a range check (dj_brdf.h:1063-1157): on a NaN direction the reference
    -- and the oracle, which restates it -- reads outside the table.  The weight of such a pair has no defined value and is not
    compared (its direction and pdf are); every other target clamps its indices and is compared everywhere."""
    if target != "utia":
        return None
    return ~(np.isfinite(i).all(1) & np.isfinite(o).all(1))


def compose(O, otarget, oproxy, oparams, u1, u2, o, target_params=None, undefined=None):
    """the definition over the oracle's separate operators -> (weight [n,3], i [n,3], pdf [n]); undefined: a mask, or a function of the
    sampled directions that returns one, of the pairs whose target value is not evaluated"""
    i = O.sample(oproxy, u1, u2, o, oparams)
    pdf = O.eval(oproxy, i, o, oparams, "pdf").astype(np.float32)
    if callable(undefined):
        undefined = undefined(i)
    if undefined is not None and undefined.any():      # see undefined_weight(): those pairs are not handed to the oracle
        fr = np.full((len(i), 3), np.nan, np.float32)
        fr[~undefined] = O.eval(otarget, i[~undefined], o[~undefined], target_params, "evalp")
    else:
        fr = O.eval(otarget, i, o, target_params, "evalp").astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = ((np.float32(1) / pdf)[:, None] * fr).astype(np.float32)
    side = i[:, 2] <= 0
    w[side] = 0
    pdf[side] = 0
    return w, i, pdf


@functools.lru_cache(maxsize=None)
def expected(target, proxy, n_bulk):
    """compose() of one pair on sampler_inputs(n_bulk), computed once and shared (read-only)"""
    import oraclelib
    o, u1, u2 = sampler_inputs(n_bulk)
    oparams = PROXIES[proxy][1] if proxy in PROXIES else None
    res = compose(oraclelib.oracle(), oracle_target(target), oracle_proxy(proxy), oparams, u1, u2, o, undefined=lambda i: undefined_weight(target, i, o))
    for a in res + (o, u1, u2):
        a.setflags(write=False)
    return res, (o, u1, u2)


def same_bits(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same(tag, got, want, target=None, o=None):
    """(weight, i, pdf) against (weight, i, pdf), bits equal, NaNs matched as NaNs; target and o: leave out the weights that
    undefined_weight() names"""
    skip = undefined_weight(target, np.asarray(want[1], np.float32), o) if target is not None else None
    for name, g, w in zip(("weight", "i", "pdf"), got, want):
        g = np.asarray(g, np.float32); w = np.asarray(w, np.float32)
        assert g.shape == w.shape, (tag, name, g.shape, w.shape)
        ok = same_bits(g, w)
        if name == "weight" and skip is not None:
            ok |= skip[:, None]
        if not ok.all():
            bad = np.argwhere(~ok)
            k = tuple(bad[0])
            raise AssertionError(f"{tag}: {name} differs in {len(bad)} of {ok.size} values, first at {k}: got {g[k]!r} want {w[k]!r}")
