"""The PARAMETER axis of the parity suites: one table of microfacet parameter sets (extreme lobes, the domain edges of every
shortcut kernel, offset and fully correlated lobes), user-supplied sgd / abc rows, and the helpers the host and GPU modules share.
No test functions here: tests/test_oracle_vs_ref.py pins the oracle to the real reference over the table,
tests/test_param_space_host.py and tests/test_gpu_param_space.py hold the product against the oracle.

Cases use oraclelib's tuple form.  Tags:
  regular     at least LIVE_FLOOR of the oracle's eval values on pairs() are finite and non-zero (asserted from the oracle alone)
  stress      in the reference's domain, but most of a batch is zero / Inf / NaN: every value is still compared, no floor
  degenerate  sets the reference answers although a limit of the model is reached (rho = +-1, radii near the float range's ends)

NOT cases: elliptic(1e-23, ...) (alpha^2 underflows to 0) and elliptic(1e19, ...) (alpha^2 overflows): the real reference ABORTS on
both ("normalize: invalid vector magnitude", dj_brdf.h:634) and the abort kills the pytest process.  Never pass a set that is not in
this table to oraclelib.reference() in-process without having run it in a child process first.
"""
import ctypes as C
import math

import numpy as np

from dj_brdf_amd import _lib, djb, param_tables, synth

N_PAIRS = (1 << 17) + 37        # >= 65536: the sharp-lobe kernel launches; + 37: the batch ends in a ragged wave
LIVE_FLOOR = 0.35               # share of finite non-zero eval values a `regular` case must reach (lowest measured: 0.37)
SHARP_ZERO_SHARE = (0.2, 0.8)   # share of all-zero results a batch inside the sharp kernel's domain must hold: both of its paths run

f32 = np.float32


def _f(x):
    return float(f32(x))


def up(x):
    """the next float above x"""
    return float(np.nextafter(f32(x), f32(np.inf)))


def dn(x):
    """the next float below x"""
    return float(np.nextafter(f32(x), f32(-np.inf)))


PI = math.pi
RHO_1M = 1.0 - 2.0 ** -24       # the largest float below 1

CASES = []


def _add(tag, *ps):
    for p in ps:
        CASES.append((tag, p))


def iso(a):
    return ("elliptic", a, a, 0.0)


# isotropic lobes; 1e-3 and 0.1 (with their float neighbours) are the edges of the sharp Beckmann kernel's domain
# (djb_kernels_eval.hip: beckmann_sharp_supported), 1e-4 / 1e4 those of contract mode, 1e-3 / 100 those of the contract sampler
_add("regular", *[iso(a) for a in (1e-3, dn(1e-3), up(1e-3), 0.0999, 0.1, dn(0.1), up(0.1), 0.1001, 1.0, 5.0)])
_add("stress", *[iso(a) for a in (1e-4, 100.0, 1e4)])
# anisotropic
_add("regular", ("elliptic", 1.0, 1e-3, 0.3))
_add("stress", ("elliptic", 1e-3, 10.0, 1.0))
# on and just over the sharp kernel's correlation edge
_add("regular", *[("pdfparams", 0.001, 0.1, r) for r in (0.99, -0.99, up(0.99), -up(0.99))])
# correlation
_add("regular", *[("pdfparams", 0.3, 0.2, r) for r in (0.99, -0.99)])
_add("stress", *[("pdfparams", 0.3, 0.2, r) for r in (0.9999, -0.9999, RHO_1M, -RHO_1M)])
_add("regular", ("pdfparams", 0.05, 0.08, 0.99), ("pdfparams", 0.05, 0.08, 0.999))
# lobes about an offset mean normal
_add("regular", ("pdfparams", 0.3, 0.2, 0.4, 0.5, -0.3), ("pdfparams", 0.3, 0.2, 0.4, 1.5, 1.0), ("pdfparams", 0.05, 0.08, 0.5, 0.2, 0.1))
_add("stress", ("pdfparams", 0.3, 0.2, 0.4, 3.0, -2.0), ("pdfparams", 0.3, 0.2, 0.4, -50.0, 0.1),
     ("pdfparams", 0.02, 0.02, 0.0, 1.0, -1.0), ("pdfparams", 0.02, 0.02, 0.0, 1e-8, 0.0))
# degenerate: djb_params_resolve writes rho == +-1.0f for the first four
_add("degenerate", ("elliptic", 1.0, 1e-4, PI / 4), ("elliptic", 1.0, 1e-4, 3 * PI / 4), ("elliptic", 2.0, 1e-5, 0.785),
     ("elliptic", 1e-4, 1.0, -PI / 4), ("elliptic", 1e-20, 1e-20, 0.3), ("elliptic", 3e-19, 3e-19, 0.0), ("elliptic", 1e6, 1e6, 0.2))
# contract mode (DJB_OPT_CONTRACT_1E5), one set just inside and one just outside every limit of
#   eval / evalp / pdf  (djb_kernels_contract.hip: ct_params):   1e-4 <= ax, ay <= 1e4, |rho| <= 0.9, no offset
#   sample              (djb_kernels_sample.hip: cts_params_ok): 1e-3 <= ax, ay <= 100, |rho| <= 0.99, |tx|, |ty| <= 10
# (ct_params' 1e-9 < ax ay sqrt(1 - rho^2) < 1e9 cannot bind inside the other limits; 1e-3, 0.99 and their neighbours are above)
_add("regular", ("pdfparams", 0.3, 0.2, 0.9), ("pdfparams", 0.3, 0.2, up(0.9)), ("pdfparams", 0.3, 0.2, -0.9), ("pdfparams", 0.3, 0.2, -up(0.9)),
     ("pdfparams", 0.05, 2.0, 0.5), ("pdfparams", 2.0, 0.05, -0.5))
_add("stress", ("pdfparams", 1e-4, 0.3, 0.0), ("pdfparams", dn(1e-4), 0.3, 0.0), ("pdfparams", 0.3, 1e-4, 0.0), ("pdfparams", 0.3, dn(1e-4), 0.0),
     ("pdfparams", 1e4, 0.3, 0.0), ("pdfparams", up(1e4), 0.3, 0.0), ("pdfparams", 0.3, 1e4, 0.0), ("pdfparams", 0.3, up(1e4), 0.0),
     ("pdfparams", 100.0, 0.3, 0.0), ("pdfparams", up(100.0), 0.3, 0.0), ("pdfparams", 0.3, dn(100.0), 0.0), ("pdfparams", 0.3, up(100.0), 0.0),
     ("pdfparams", 0.3, 0.2, 0.4, 10.0, 0.0), ("pdfparams", 0.3, 0.2, 0.4, up(10.0), 0.0), ("pdfparams", 0.3, 0.2, 0.4, 0.0, -10.0),
     ("pdfparams", 0.3, 0.2, 0.4, 0.0, -up(10.0)))

CASES = [(tag, (p[0],) + tuple(_f(v) for v in p[1:])) for tag, p in CASES]
assert len(set(p for _, p in CASES)) == len(CASES)


def case_id(case):
    tag, p = case
    return tag[:3] + "-" + p[0][:3] + "-" + "_".join("%.9g" % v for v in p[1:])       # %.9g: float neighbours keep distinct names


FRESNEL_IDEAL = ("ideal",)
FRESNEL_SCHLICK = ("schlick", 1.0, 0.71, 0.29)
FRESNEL_UNPOLARIZED = ("unpolarized", 1.5, 1.8, 2.4)


# ---------------------------------------------------------------- the domains of the shortcut kernels, restated from their predicates
def resolved(oracle, p):
    """(ax, ay, rho, tx, ty) as the reference's params object holds them (floats)"""
    return tuple(f32(v) for v in oracle.params_get(p)[6:11])


def in_sharp_domain(oracle, p):
    """beckmann_sharp_supported (djb_kernels_eval.hip), the parameter part; the three Fresnel terms used here are all inside"""
    ax, ay, rho, tx, ty = resolved(oracle, p)
    return bool(tx == 0 and ty == 0 and ax >= f32(1e-3) and ay >= f32(1e-3) and ax <= f32(0.1) and ay <= f32(0.1) and abs(rho) <= f32(0.99))


def in_contract_domain(oracle, p):
    """ct_params (djb_kernels_contract.hip), the parameter part"""
    ax, ay, rho, tx, ty = resolved(oracle, p)
    if not (tx == 0 and ty == 0 and abs(rho) <= f32(0.9) and f32(1e-4) <= ax <= f32(1e4) and f32(1e-4) <= ay <= f32(1e4)):
        return False
    s = f32(np.sqrt(1.0 - float(f32(rho * rho))))
    return bool(1e-9 < float(ax) * float(ay) * float(s) < 1e9)


def in_sample_contract_domain(oracle, p):
    """cts_params_ok (djb_kernels_sample.hip)"""
    ax, ay, rho, tx, ty = resolved(oracle, p)
    return bool(f32(1e-3) <= ax <= f32(1e2) and f32(1e-3) <= ay <= f32(1e2) and abs(rho) <= f32(0.99) and abs(tx) <= f32(10) and abs(ty) <= f32(10))


# ---------------------------------------------------------------- inputs and comparisons
def value_bits(a):
    """the bits of every value, signs of zeros included; NaNs (whose payload is the processor's business) as one pattern"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def pairs(oracle, ob, p, n=N_PAIRS):
    """(i, o, u1, u2): the bench directions, every second i replaced by the oracle's own sample of the lobe for that o -- the reference
    itself places half the pairs inside the lobe.  Without this a Beckmann lobe at alpha = 1e-4 is all zeros and a comparison vacuous.

    For a set inside the sharp Beckmann kernel's domain every fourth i (of the half left alone) is o mirrored about a half vector 60 degrees
    off the normal: exp(-tan^2 / alpha^2) is an exact zero there for every alpha of that domain (tan^2 60 / 0.1^2 = 300 > 104).  The bench
    directions alone leave only 0.09 of a batch all-zero at alpha = 0.1, short of SHARP_ZERO_SHARE: the kernel's trivial path would see
    too few pairs, and hardly a wave made of them only."""
    i, o = synth.directions_aos(n, synth.SEED_I).copy(), synth.directions_aos(n, synth.SEED_O)
    u1, u2 = synth.uniforms(n, synth.SEED_U1), synth.uniforms(n, synth.SEED_U2)
    i[1::2] = oracle.sample(ob, u1, u2, o, p)[1::2]
    if in_sharp_domain(oracle, p):
        phi = np.arctan2(i[0::4, 1], i[0::4, 0]).astype(np.float64)
        h = np.stack([np.sin(PI / 3) * np.cos(phi), np.sin(PI / 3) * np.sin(phi), np.full_like(phi, np.cos(PI / 3))], 1)
        oo = o[0::4].astype(np.float64)
        i[0::4] = (2.0 * np.sum(oo * h, axis=1, keepdims=True) * h - oo).astype(np.float32)
    return i, o, u1, u2


def oracle_outputs(oracle, ob, inputs, p):
    i, o, u1, u2 = inputs
    want = {op: oracle.eval(ob, i, o, p, op) for op in ("eval", "evalp", "pdf")}
    want["sample"] = oracle.sample(ob, u1, u2, o, p)
    want["is_w"], want["is_i"], want["is_pdf"] = oracle.evalp_is(ob, u1, u2, o, p)
    return want


def live_share(want_eval):
    with np.errstate(invalid="ignore"):
        return float(np.mean(np.isfinite(want_eval) & (want_eval != 0)))


def zero_share(want_eval):
    return float(np.mean(np.all(want_eval == 0, axis=1)))


def assert_reference_side_conditions(oracle, ndf, case, want_eval):
    """what makes a comparison on this case worth something, from the oracle's output alone"""
    tag, p = case
    if tag == "regular":
        s = live_share(want_eval)
        assert s >= LIVE_FLOOR, f"{ndf} {p}: only {s:.3f} of the oracle's eval values are finite and non-zero: not a `regular` case"
    if ndf == "beckmann" and in_sharp_domain(oracle, p):
        z = zero_share(want_eval)
        assert SHARP_ZERO_SHARE[0] <= z <= SHARP_ZERO_SHARE[1], f"beckmann {p}: {z:.3f} of the results are all-zero: one path of the sharp kernel goes unexercised"


def mk_fresnel(f):
    if f[0] == "ideal": return djb.fresnel.ideal()
    if f[0] == "schlick": return djb.fresnel.schlick(f[1:4])
    return djb.fresnel.unpolarized(f[1:4])


def mk_params(p):
    return getattr(djb.microfacet.params, p[0])(*p[1:])


class Cached(C.Structure):
    """include/djb_hip.h: djb_params_cached"""
    _fields_ = [("p", _lib.Params), ("r", _lib.ParamsResolved)]


def mk_cached(p):
    """the same set as a djb_params that carries its resolved form (kind | DJB_PARAMS_RESOLVED_FOLLOWS): what the C++ facade's params
    objects hand to every call"""
    c = Cached(); c.p = mk_params(p)._p
    _lib.check(_lib.load().djb_params_resolve(C.byref(c.p), C.byref(c.r)))
    c.p.kind |= 0x100
    q = djb.microfacet.params.standard(); q._p = c.p; q._keep = c      # the mirror passes byref(_p): a view into `c`, so `r` follows it in memory
    return q


def fresnels_for(oracle, p):
    """(fresnel, shadow) set-ups of a case: ideal and Schlick; inside the sharp kernel's domain also its third Fresnel term and no shadowing"""
    fs = [(FRESNEL_IDEAL, True), (FRESNEL_SCHLICK, True)]
    if in_sharp_domain(oracle, p):
        fs += [(FRESNEL_UNPOLARIZED, True), (FRESNEL_IDEAL, False)]
    return fs


def product_outputs(g, inputs, up_, conv_in=lambda a: a, conv_out=np.asarray, fused=True):
    """every operator that takes parameters, through the product's object `g`; (None | status name and message, outputs as [n, 3] / [n] numpy arrays)"""
    i, o, u1, u2 = inputs
    di, do = conv_in(i), conv_in(o)
    out = {}
    try:
        for op in ("eval", "evalp", "pdf"):
            out[op] = conv_out(getattr(g, op)(di, do, up_))
        if fused:
            fr, pdf = g.eval_pdf(di, do, up_)
            out["fused_eval"], out["fused_pdf"] = conv_out(fr), conv_out(pdf)
            fr, pdf = g.eval_pdf(di, do, up_, cos=True)
            out["fused_evalp"] = conv_out(fr)
        out["sample"] = conv_out(g.sample(u1, u2, do, up_))
        w, si, pdf = g.evalp_is(u1, u2, do, up_)
        out["is_w"], out["is_i"], out["is_pdf"] = conv_out(w), conv_out(si), conv_out(pdf)
    except djb.exc as e:
        return f"{e.status_name}: {e}", out
    return None, out


WANT_OF = {"fused_eval": "eval", "fused_pdf": "pdf", "fused_evalp": "evalp"}


def assert_outputs_equal(name, got, want):
    for k, v in got.items():
        w = want[WANT_OF.get(k, k)]
        assert v.shape == w.shape, (name, k, v.shape, w.shape)
        bad = value_bits(v) != value_bits(w)
        if bad.any():
            first = int(np.flatnonzero(bad.reshape(bad.shape[0], -1).any(axis=1))[0])
            raise AssertionError(f"{name}: {k}: {int(bad.sum())} of {bad.size} values differ from the oracle's bits; first at unit {first}: "
                                 f"got {np.atleast_1d(v[first])} want {np.atleast_1d(w[first])}")


# ---------------------------------------------------------------- user-supplied sgd / abc rows
def _published(kind):
    names = synth.MERL_NAMES
    return np.array([getattr(param_tables, kind + "_params")(n) for n in names], np.float64)


def resampled_rows(kind, count=60, seed=20260):
    """rows nobody published but in range: every column drawn independently from the published values of that column"""
    tab = _published(kind)
    rng = np.random.default_rng(seed + (0 if kind == "sgd" else 1))
    pick = rng.integers(0, tab.shape[0], size=(count, tab.shape[1]))
    return [tab[pick[r], np.arange(tab.shape[1])].copy() for r in range(count)]


def _sgd_with(base, **cols):
    row = np.array(param_tables.sgd_params(base), np.float64)
    for name, v in cols.items():
        k = param_tables.SGD_FIELDS.index(name)
        row[3 * k:3 * k + 3] = v
    return row


def sgd_edge_rows():
    """rows on and over the limits of the sgd fast tier's domain (djb_fast_models.inc: sgd_fast_row):
    1 <= k <= 4096, |theta0| <= 4, 1e-200 <= lambda <= 1e100, 1e-300 <= c <= 1e300, 1e-12 <= alpha <= 1e12, 0 <= p <= 1024, 1e-100 <= kappa <= 1e100"""
    b = "gold-metallic-paint"
    return [("k=1", _sgd_with(b, k=1.0)), ("k=4096", _sgd_with(b, k=4096.0)), ("k=4097", _sgd_with(b, k=4097.0)), ("k=0.5", _sgd_with(b, k=0.5)),
            ("k mixed", _sgd_with(b, k=(1.0, 4096.0, 17.5))),
            ("theta0=4", _sgd_with(b, theta0=4.0)), ("theta0=-4", _sgd_with(b, theta0=-4.0)), ("theta0=1.5707", _sgd_with(b, theta0=1.5707)),
            ("theta0 beyond 4", _sgd_with(b, theta0=(4.5, -4.5, 0.1))),
            ("lambda=1e-300", _sgd_with(b, **{"lambda": 1e-300})), ("lambda=1.5e7", _sgd_with(b, **{"lambda": 1.5e7})),
            ("c=3e-8", _sgd_with(b, c=3e-8)), ("c=1e38", _sgd_with(b, c=1e38)),
            ("alpha=1e-12", _sgd_with(b, alpha=1e-12)), ("alpha=1e12", _sgd_with(b, alpha=1e12)), ("alpha=1e-6 p=1024", _sgd_with(b, alpha=1e-6, p=1024.0)),
            ("p=1025", _sgd_with(b, p=1025.0)), ("p=0", _sgd_with(b, p=0.0)),
            ("kappa=1e-100", _sgd_with(b, kap=1e-100)), ("kappa=1e100", _sgd_with(b, kap=1e100)), ("kappa=1e-101", _sgd_with(b, kap=1e-101))]


def _abc_with(base, **cols):
    row = np.array(param_tables.abc_params(base), np.float64)
    at = {"kD": slice(0, 3), "A": slice(3, 6), "B": 6, "C": 7, "ior": 8}
    for name, v in cols.items():
        row[at[name]] = v
    return row


def abc_edge_rows():
    """rows on and over the limits of the abc fast tier (djb_fast_models.inc: abc_ndf_fast): 0 <= C <= 4096, 2^-100 <= w = 1 + B (1 - cos) <= 2^100,
    |C ln w| < 700 -- the last two depend on the direction, so a row can be inside for part of a batch only"""
    b = "gold-metallic-paint"
    return [("C=0", _abc_with(b, C=0.0)), ("C=4096", _abc_with(b, C=4096.0)), ("C=4097", _abc_with(b, C=4097.0)), ("C=-0.5", _abc_with(b, C=-0.5)),
            ("B=1e-300", _abc_with(b, B=1e-300)), ("B=1e30", _abc_with(b, B=1e30)), ("B=1e31", _abc_with(b, B=1e31)), ("B=1e300", _abc_with(b, B=1e300)),
            ("C ln w to 690", _abc_with(b, B=1e3, C=99.0)), ("C ln w over 700", _abc_with(b, B=1e3, C=103.0)), ("C=4096 B=1e-3", _abc_with(b, B=1e-3, C=4096.0)),
            ("A=1e38", _abc_with(b, A=1e38)), ("A=1e-40", _abc_with(b, A=(1e-40, 1e-30, 1e-45))), ("ior=1.0001", _abc_with(b, ior=1.0001)),
            ("ior=50", _abc_with(b, ior=50.0))]


def oracle_model(oracle, kind, row):
    """the oracle's object of an explicit row: the path oracle.sgd(name) / oracle.abc(name) take with a published row"""
    row = np.ascontiguousarray(row, np.float64)
    return C.c_void_p(oracle._fn("create_" + kind)(row.ctypes.data_as(C.c_void_p)))


def model_pairs(n=1 << 16):
    return synth.directions_aos(n, synth.SEED_I, 31), synth.directions_aos(n, synth.SEED_O, 31)
