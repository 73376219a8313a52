"""Cases of the light-sample call on a single object (brdf.evalp_pdf_proxy / djb_evalp_pdf_proxy_batch): for GIVEN pairs, evalp of the
target (merl, utia, sgd, abc) and the pdf of the proxy (a fitted lobe), both 0 where i or o is not above the horizon
(mitsuba/dj_merl.cpp:33-42, 64-65: eval() and pdf() of the plugins).

Expected values never come from the product.  They are the ORACLE's separate operators
    fr  = O.eval(target, i, o, None, "evalp")        and        pdf = O.eval(proxy, i, o, params, "pdf")
both zeroed where i.z <= 0 or o.z <= 0 (a numpy comparison: a NaN z does not zero); compared as bits, NaNs matched as NaNs.

utia is the one target with undefined values: its reference indexes the table without a range check, so a pair with a non-finite
component is not handed to the oracle and its fr is not compared (proxy_is_cases.undefined_weight); its pdf is.

Inputs (N = 40 001): merl_set_light_cases.inputs() -- hits with o.z < 0, with i.z < 0, NaN components, zero vectors, the on-normal block
and the pairs around the mirror direction that give sharp lobes a non-zero pdf."""
import functools

import numpy as np

import merl_set_light_cases as light
import proxy_is_cases as pis

TARGETS, PROXIES, GPU_PAIRS = pis.TARGETS, pis.PROXIES, pis.GPU_PAIRS
product_target, product_proxy, product_params = pis.product_target, pis.product_proxy, pis.product_params
oracle_target, oracle_proxy, undefined_weight, same_bits = pis.oracle_target, pis.oracle_proxy, pis.undefined_weight, pis.same_bits
inputs, guarded, declined_block = light.inputs, light.guarded, light.declined_block

N = light.N
GUARD_MIN = 500                 # pairs that take the guard through i.z <= 0, and through o.z <= 0
NAN_Z_MIN = 50                  # pairs with a NaN z
LIVE_MIN = 10_000               # per proxy: pairs with a finite pdf > 0; per target: pairs with a non-zero fr
UNDEFINED_MAX = 0.01            # share of the pairs whose utia value is undefined


def oracle_params(proxy):
    return PROXIES[proxy][1] if proxy in PROXIES else None


def oracle_fr(O, target, i, o, target_params=None):
    """evalp of the target, zeroed under the guard; NaN where the target's value is undefined (not handed to the oracle)"""
    undefined = undefined_weight(target, i, o)
    with np.errstate(all="ignore"):
        if undefined is not None and undefined.any():
            fr = np.full((len(i), 3), np.nan, np.float32)
            fr[~undefined] = O.eval(oracle_target(target), i[~undefined], o[~undefined], target_params, "evalp")
        else:
            fr = np.array(O.eval(oracle_target(target), i, o, target_params, "evalp"), np.float32)
    fr[guarded(i, o)] = 0.0
    return fr


def oracle_pdf(O, proxy, i, o, params):
    """the proxy's pdf, zeroed under the guard"""
    with np.errstate(all="ignore"):
        pdf = np.array(O.eval(oracle_proxy(proxy), i, o, params, "pdf"), np.float32).reshape(-1)
    pdf[guarded(i, o)] = 0.0
    return pdf


@functools.lru_cache(maxsize=None)
def expected_fr(target):
    """[N, 3] on inputs(), computed once (read-only)"""
    import oraclelib
    fr = oracle_fr(oraclelib.oracle(), target, *inputs())
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def expected_pdf(proxy):
    """[N] on inputs(), computed once (read-only)"""
    import oraclelib
    pdf = oracle_pdf(oraclelib.oracle(), proxy, *inputs(), oracle_params(proxy))
    pdf.setflags(write=False)
    return pdf


def expected(target, proxy):
    return expected_fr(target), expected_pdf(proxy)


def expected_on(O, target, proxy, i, o, params=None, target_params=None):
    """(fr, pdf) on other pairs; params: the oracle's parameter tuple of the proxy (default: the named proxy's)"""
    return oracle_fr(O, target, i, o, target_params), oracle_pdf(O, proxy, i, o, params if params is not None else oracle_params(proxy))


def assert_same(tag, got, want, target=None, i=None, o=None):
    """(fr, pdf) against (fr, pdf), bits equal, NaNs matched as NaNs; target, i and o: leave out the fr that undefined_weight() names"""
    skip = undefined_weight(target, np.asarray(i, np.float32), np.asarray(o, np.float32)) if target is not None else None
    for name, g, w in zip(("fr", "pdf"), got, want):
        g = np.asarray(g, np.float32); w = np.asarray(w, np.float32)
        assert g.shape == w.shape, (tag, name, g.shape, w.shape)
        ok = same_bits(g, w)
        if name == "fr" and skip is not None:
            ok |= skip[:, None]
        if not ok.all():
            bad = np.argwhere(~ok)
            k = tuple(bad[0])
            raise AssertionError(f"{tag}: {name} differs in {len(bad)} of {ok.size} values, first at {k}: got {g[k]!r} want {w[k]!r}")


def assert_input_conditions():
    """what the inputs must exercise, on oracle values only"""
    i, o = inputs()
    with np.errstate(invalid="ignore"):
        assert int((i[:, 2] <= 0).sum()) >= GUARD_MIN and int((o[:, 2] <= 0).sum()) >= GUARD_MIN
    assert int((np.isnan(i[:, 2]) | np.isnan(o[:, 2])).sum()) >= NAN_Z_MIN
    z = guarded(i, o)
    undefined = undefined_weight("utia", i, o)
    assert 0 < undefined.mean() <= UNDEFINED_MAX, undefined.mean()
    for target in TARGETS:
        assert undefined_weight(target, i, o) is None or target == "utia"
    for proxy in sorted({p for _, p in GPU_PAIRS}):
        pdf = expected_pdf(proxy)
        n_pdf = int((np.isfinite(pdf) & (pdf > 0) & ~z).sum())
        assert n_pdf >= LIVE_MIN, (proxy, n_pdf)
        assert not pdf[z].view(np.uint32).any(), proxy
    for target in TARGETS:
        fr = expected_fr(target)
        n_fr = int(((np.nan_to_num(fr) != 0).any(1) & ~z).sum())
        assert n_fr >= LIVE_MIN, (target, n_fr)
        assert not fr[z].view(np.uint32).any(), target
