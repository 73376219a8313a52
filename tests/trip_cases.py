"""Cases for the second and third grid-stride trips of the core kernels (csrc/djb_kernels_eval.hip, csrc/djb_kernels_sample.hip, k_utia_v2) and for
the values of every core operator at awkward sizes and placements.  No test functions here: tests/test_trip_cases_host.py pins the cases on
the CPU, tests/test_gpu_trips.py and tests/test_gpu_batch_values.py run them on the device.

Pattern (as tests/test_gpu_wave_queue.py): a 4 096-unit block of inputs; the ORACLE's result on the block, once per (object, operator, parameter
set), cached and read-only; the block tiled and cut to n units; all n units compared as bits (param_space_cases.value_bits: signs of zeros
count, NaNs are one pattern).  Expected values never come from the product.

Every trip size is a multiple of 4 096, so with n = (trips - 1) * TRIP + 4096 - 179 the sixteen workgroups that take the last trip (eight of 512 ...)
see exactly the block again, minus a ragged 179, and each of their waves meets the same 64 inputs on every trip.

Trip sizes, restated from the launch code (tests/test_trip_cases_host.py holds them against the formulas restated below):
  capped     4096 * 256    k_eval / k_sample of tabular, sgd, abc, lambert, merl (exact only), utia (exact only), k_sample of tabular_anisotropic,
                           the harness kernels, the contract fix-up's rescan: GRID_CAP = 256 * 16 workgroups of BLOCK = 256
  aniso_eval 2048 * 1024   k_eval<TABULAR_ANISO>: eval_block = 1024, at most 2048 workgroups (launch_eval_kind_fr)
  sharp      4096 * 256    k_eval_bk_sharp: `blocks` of launch_eval_kind_fr
  sampler    5120 * 256    k_sample_bk: grid_persistent (csrc/djb_kernels_sample.hip)
  utia_v2    16384 * 256   k_utia_v2: GRID_CAP = 256 * 64 (csrc/djb_kernels_utia.hip)

The two queue blocks.  Both kernels keep a per-wave LDS queue of deferred units; a wave that queues c units per trip carries a residue from trip to
trip.  Wave w of the block (64 waves) queues WAVE_COUNTS[w] of its 64 lanes, chosen by a seeded permutation (the ballot prefix count matters):
  c = 0
  1 <= c <= 31    the residue survives two trips and is only flushed at the end; in three trips 22 <= c <= 31 drains on the third
  32 <= c <= 63   the drain in trip 2 mixes entries of both trips and leaves 2c - 64 behind
  c = 64

sharp_block(): the queued pairs are exactly the non-trivial ones of k_eval_bk_sharp, for every lobe of SHARP_LOBES, either Fresnel term, shadowing on or off:
  trivial  o below the horizon (rule (a)), or a finite pair, both directions at most 15 degrees from a half vector 50-70 degrees off the normal: polar
           angles <= 85 degrees (z >= 0.087) and r^2 = s' Sigma^-1 s >= tan^2(50 deg) / lambda_max(Sigma) >= 1.42 / 0.01 = 142 >= 104 (rule (b));
           lambda_max(Sigma) <= ax^2 + ay^2 <= 0.0104 for the three lobes.  (Not from 40 degrees: tan^2(40 deg) / 0.0104 = 68 is short of 104.)
  queued   o a bench direction with z >= 0.3, i its mirror image about a half vector whose slope is at most 0.01: r^2 <= 1e-4 / lambda_min(Sigma)
           <= 1e-4 / 3.9e-4 < 0.26, D is of order 1 / (pi ax ay); a few pairs with a NaN or an infinite component in i, which rule (b) (`sane`)
           sends to the exact path and for which the oracle returns NaN.
sampler_block(): the deferred samples of k_sample_bk, by flag site (csrc/djb_kernels_sample.hip):
  o == (0, 0, 1)          bk_sample_common, R_DEGENERATE: k = (0, 0, 1) for a lobe without offset, !(k.z < 1)
  o.z < 0                 bk_sample_common, R_DEGENERATE: !(k.z > 0) (c = o.z for a lobe without offset)
  u2 <= 1e-3 or >= 1-1e-3 erfinv_central<false> at R_TAIL_QF1: u = 2 (0.99998 u2 + 1e-5) - 1 has 1 - u^2 <= 4.1e-3 < exp(-5), so !(w < 5)
  u2 NaN                  the same site: logf_main<true> flags R_LOGF for a NaN operand, and !(w < 5) holds for a NaN w
  the other lanes hold bench samples, of which the kernel defers some for reasons of its own (a fifth Newton trip, a guard band): the count of a wave is
  WAVE_COUNTS[w] plus a few.  Counted per wave on a measurement build of the kernel (DJB_EXP_RARE_COUNT, not part of the library): no wave below its
  WAVE_COUNTS; elliptic(0.2, 0.5, 0.7): 0-3 more per wave, 35 over the block, all four classes occur (7 waves keep an empty queue); the default lobe: 0-8
  more per wave, 194 over the block, every wave defers something (the classes 1-31, 32-63 and 64 occur)."""
import ctypes as C
import functools

import numpy as np

import utia_set_cases
from dj_brdf_amd import _lib, djb, synth
from param_space_cases import FRESNEL_IDEAL, FRESNEL_SCHLICK, FRESNEL_UNPOLARIZED, mk_fresnel, mk_params, value_bits
from test_gpu_parity import hostile_pairs

BLOCK_N = 4096
RAGGED = 179

# ------------------------------------------------------------------ launch shapes, restated
WG = 256                       # BLOCK, djb_kernels_eval.hip:14 and djb_kernels_sample.hip:27
EVAL_GRID_CAP = 256 * 16       # GRID_CAP, djb_kernels_eval.hip:16
ANISO_WG, ANISO_GRID = 1024, 2048      # eval_block, djb_kernels_eval.hip:47; the workgroup limit of launch_eval_kind_fr, djb_kernels_eval.hip:232
SHARP_GRID = 4096              # launch_eval_kind_fr, djb_kernels_eval.hip:237-238
SAMPLER_GRID, SAMPLER_TILES_PER_WG = 5120, 48      # grid_persistent, djb_kernels_sample.hip:56-65
UTIA_GRID_CAP = 256 * 64       # GRID_CAP, djb_kernels_utia.hip:16 (launch: djb_kernels_utia.hip:190)

TRIP = {"capped": EVAL_GRID_CAP * WG, "aniso_eval": ANISO_GRID * ANISO_WG, "sharp": SHARP_GRID * WG, "sampler": SAMPLER_GRID * WG, "utia_v2": UTIA_GRID_CAP * WG}


def grid_capped(n, block, cap):
    """djbk::grid_capped, djb_internal.hpp:17-23"""
    return max(1, min(-(-n // block), cap))


def grid_aniso_eval(n):
    """launch_eval_kind_fr, djb_kernels_eval.hip:232"""
    return max(1, min(-(-n // ANISO_WG), ANISO_GRID))


def grid_sharp(n):
    """`blocks` of launch_eval_kind_fr, djb_kernels_eval.hip:237-239"""
    tiles = -(-n // WG)
    blocks = (tiles + 31) // 32
    if blocks < 4096:
        blocks = min(tiles, 4096)
    return min(blocks, 0x7fffffff)


def grid_persistent(n):
    """grid_persistent, djb_kernels_sample.hip:57-65"""
    tiles = -(-n // WG)
    blocks = -(-tiles // SAMPLER_TILES_PER_WG)
    if blocks < 5120:
        blocks = min(tiles, 5120)
    return max(1, min(blocks, 0x7fffffff))


def units(family, trips=2):
    """n of a run that ends in a ragged trip number `trips`"""
    return (trips - 1) * TRIP[family] + BLOCK_N - RAGGED


def tiled(a, n):
    """the block repeated and cut to n units"""
    return np.concatenate([a] * -(-n // len(a)))[:n]


# ------------------------------------------------------------------ per-wave queue counts
def _wave_counts():
    low = [1, 2, 3, 5, 8, 11, 13, 16, 19, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31]
    high = [32, 33, 34, 35, 37, 40, 42, 43, 45, 47, 48, 50, 52, 55, 57, 59, 60, 61, 62, 63]
    c = np.array([0] * 12 + low + high + [64] * 12)
    c = c[np.random.default_rng(6464).permutation(64)]
    c.setflags(write=False)
    return c


WAVE_COUNTS = _wave_counts()          # [64]: queued lanes of wave w of the block


def wave_class(c):
    return 0 if c == 0 else 1 if c <= 31 else 2 if c <= 63 else 3


@functools.lru_cache(maxsize=None)
def queued_lanes(seed):
    """[4096] bool: WAVE_COUNTS[w] lanes of wave w, by a seeded permutation"""
    rng = np.random.default_rng(seed)
    q = np.zeros(BLOCK_N, bool)
    for w, c in enumerate(WAVE_COUNTS):
        q[64 * w + rng.permutation(64)[:c]] = True
    q.setflags(write=False)
    return q


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def bench_block():
    return (synth.directions_aos(BLOCK_N, synth.SEED_I), synth.directions_aos(BLOCK_N, synth.SEED_O),
            synth.uniforms(BLOCK_N, synth.SEED_U1), synth.uniforms(BLOCK_N, synth.SEED_U2))


# ------------------------------------------------------------------ the sharp-lobe block
SHARP_LOBES = (("elliptic", 0.05, 0.05, 0.0), ("elliptic", 0.02, 0.1, 0.3), ("pdfparams", 0.05, 0.08, 0.5, 0.0, 0.0))     # of test_gpu_parity.SHARP_PARAMS
SHARP_SETUPS = tuple((f, s) for f in (FRESNEL_IDEAL, FRESNEL_SCHLICK) for s in (True, False))
SHARP_SEED = 20261


def _mirror(o, h):
    return 2.0 * np.sum(o * h, axis=1, keepdims=True) * h - o


@functools.lru_cache(maxsize=None)
def sharp_block():
    """(i, o [4096, 3] float32, queued [4096] bool), read-only"""
    rng = np.random.default_rng(SHARP_SEED)
    queued = queued_lanes(SHARP_SEED)
    bi, bo, _, _ = bench_block()
    n = BLOCK_N
    # trivial, rule (b): both directions 0-15 degrees from a half vector 50-70 degrees off the normal, mirror images of each other about it
    th, ph = np.deg2rad(rng.uniform(50, 70, n)), rng.uniform(0, 2 * np.pi, n)
    h = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1)
    t = np.stack([np.cos(th) * np.cos(ph), np.cos(th) * np.sin(ph), -np.sin(th)], 1)            # two unit tangents at h
    b = np.stack([-np.sin(ph), np.cos(ph), np.zeros(n)], 1)
    td, pd = np.deg2rad(rng.uniform(0, 15, n))[:, None], rng.uniform(0, 2 * np.pi, n)[:, None]
    o = np.cos(td) * h + np.sin(td) * (np.cos(pd) * t + np.sin(pd) * b)
    i = _mirror(o, h)
    # trivial, rule (a): o below the horizon, i a bench direction
    a = ~queued & (rng.random(n) < 0.4)
    o[a] = bo[a] * np.array([1, 1, -1]); i[a] = bi[a]
    # queued: o a bench direction with z >= 0.3, i its mirror image about a half vector of slope <= 0.01
    oq = bo.astype(np.float64)
    flat = oq[:, 2] < 0.3
    oq[flat] = oq[flat] * np.array([0.5, 0.5, 0]) + np.array([0, 0, 0.8]); oq /= np.linalg.norm(oq, axis=1, keepdims=True)
    s, ps = rng.uniform(0, 0.01, n), rng.uniform(0, 2 * np.pi, n)
    hq = np.stack([-s * np.cos(ps), -s * np.sin(ps), np.ones(n)], 1); hq /= np.linalg.norm(hq, axis=1, keepdims=True)
    o[queued] = oq[queued]; i[queued] = _mirror(oq, hq)[queued]
    i, o = i.astype(np.float32), o.astype(np.float32)
    # a few of the queued pairs with a NaN / an infinite component: rule (b)'s `sane` fails, the exact path answers
    bad = np.flatnonzero(queued)[::97]
    i[bad[0::3], 0] = np.nan; i[bad[1::3], 1] = np.nan; i[bad[2::3], 2] = np.inf
    return _frozen(i, o, queued)


# ------------------------------------------------------------------ the Beckmann sampler's block
SAMPLER_PARAMS = (("elliptic", 0.2, 0.5, 0.7), None)
SAMPLER_SEED = 20262


@functools.lru_cache(maxsize=None)
def sampler_block():
    """(u1, u2 [4096], o [4096, 3] float32, deferred [4096] bool), read-only"""
    rng = np.random.default_rng(SAMPLER_SEED)
    deferred = queued_lanes(SAMPLER_SEED)
    _, o, u1, u2 = (a.copy() for a in bench_block())
    fam = rng.integers(0, 5, BLOCK_N)
    sel = lambda f: deferred & (fam == f)
    o[sel(0)] = (0, 0, 1)                                                                       # R_DEGENERATE: k.z == 1
    o[sel(1), 2] *= -1                                                                          # R_DEGENERATE: k.z <= 0 (bench z > 0)
    u2[sel(2)] = (rng.random(BLOCK_N, dtype=np.float32) * np.float32(1e-3))[sel(2)]             # R_TAIL_QF1, lower tail
    u2[sel(3)] = (np.float32(1) - rng.random(BLOCK_N, dtype=np.float32) * np.float32(1e-3))[sel(3)]      # R_TAIL_QF1, upper tail
    u2[sel(4)] = np.nan                                                                         # R_LOGF / R_TAIL_QF1
    assert (o[sel(1), 2] < 0).all()
    return _frozen(u1, u2, o, deferred)


# ------------------------------------------------------------------ blocks of the other kinds
@functools.lru_cache(maxsize=None)
def hostile_block():
    """(i, o, u1, u2): test_gpu_parity.hostile_pairs of the 4 096 bench pairs (families of 256: either direction below / on the horizon, un-normalised,
    opposed, grazing, on the normal, equal, NaN / Inf / zero vectors, h on the normal) and uniforms outside [0, 1) / NaN, as tools/hostile_parity_sweep.py"""
    d = bench_block()
    i, o = hostile_pairs(d)
    u1, u2 = d[2].copy(), d[3].copy()
    u1[2600:2608] = np.nan; u2[2608:2616] = np.nan; u1[2616:2624] = -0.5; u2[2624:2632] = 1.5; u1[2632:2640] = 1.0; u2[2640:2648] = 0.0
    u1[2648:2656] = 0.0; u2[2656:2664] = 1.0
    return _frozen(i, o, u1, u2)


@functools.lru_cache(maxsize=None)
def finite_block():
    """(i, o, u1, u2): the grid-line directions of utia_set_cases.grid_block (finite, above the horizon): a UTIA value is defined for every pair"""
    _, i, o = utia_set_cases.grid_block()
    return i, o, bench_block()[2], bench_block()[3]


BLOCKS = {"sharp": lambda: sharp_block()[:2] + bench_block()[2:], "sampler": lambda: (bench_block()[0], sampler_block()[2], sampler_block()[0], sampler_block()[1]),
          "hostile": hostile_block, "finite": finite_block}


# ------------------------------------------------------------------ objects: one spec, the product's object and the oracle's
# spec: ("mf", ndf, fresnel, shadow) | "tabular" | "aniso" | "sgd" | "abc" | "lambert" | "merl" | "utia" | "utia_drawn"
SGD_NAME, ABC_NAME = "gold-metallic-paint", "chrome"          # as tests/test_gpu_bounds.py


def product_object(spec, ctx):
    if isinstance(spec, tuple):
        return getattr(djb, spec[1])(mk_fresnel(spec[2]), spec[3], ctx=ctx)
    if spec == "tabular":
        return djb.tabular(djb.merl.from_table(synth.merl_table(), ctx=ctx), 90, True, ctx=ctx)
    if spec == "aniso":
        return djb.tabular_anisotropic(djb.utia.from_table(utia_set_cases.tables()[0], ctx=ctx), 10, 14, True, ctx=ctx)
    if spec == "sgd":
        return djb.sgd(SGD_NAME, ctx=ctx)
    if spec == "abc":
        return djb.abc(ABC_NAME, ctx=ctx)
    if spec == "lambert":
        return djb.lambert(ctx=ctx)
    if spec == "merl":
        return djb.merl.from_table(synth.merl_table(), ctx=ctx)
    return djb.utia.from_table(utia_set_cases.tables()[{"utia": 0, "utia_drawn": 1}[spec]], ctx=ctx)


@functools.lru_cache(maxsize=None)
def oracle_object(spec):
    import oraclelib
    O = oraclelib.oracle()
    if isinstance(spec, tuple):
        return O.microfacet(spec[1], spec[2], spec[3])
    if spec == "tabular":
        return O.tabular(O.merl_from_table(synth.merl_table()), 90, True)
    if spec == "aniso":
        return O.tabular_anisotropic(utia_set_cases.oracle_materials()[0], 10, 14, True)
    if spec == "sgd":
        return O.sgd(SGD_NAME)
    if spec == "abc":
        return O.abc(ABC_NAME)
    if spec == "lambert":
        return O.lambert()
    if spec == "merl":
        return O.merl_from_table(synth.merl_table())
    return utia_set_cases.oracle_materials()[{"utia": 0, "utia_drawn": 1}[spec]]


# operator -> the oracle outputs it returns, in the order of the product's outputs
OPS = {"eval": ("eval",), "evalp": ("evalp",), "pdf": ("pdf",), "eval_pdf0": ("eval", "pdf"), "eval_pdf1": ("evalp", "pdf"), "sample": ("sample",),
       "evalp_is": ("is_w", "is_i", "is_pdf")}
EVAL_OPS = ("eval", "evalp", "pdf", "eval_pdf0", "eval_pdf1")
SAMPLE_OPS = ("sample", "evalp_is")


@functools.lru_cache(maxsize=None)
def _oracle_group(spec, block, params, group):
    import oraclelib
    O = oraclelib.oracle()
    ob = oracle_object(spec)
    i, o, u1, u2 = BLOCKS[block]()
    if group in ("eval", "evalp", "pdf"):
        out = {group: O.eval(ob, i, o, params, group)}
    elif group == "sample":
        out = {"sample": O.sample(ob, u1, u2, o, params)}
    else:
        out = dict(zip(("is_w", "is_i", "is_pdf"), O.evalp_is(ob, u1, u2, o, params)))
    out = {k: np.ascontiguousarray(a, np.float32) for k, a in out.items()}
    _frozen(*out.values())
    return out


def oracle_output(spec, block, params, name):
    """one output of the ORACLE on a block (computed once, read-only): eval / evalp [4096, 3], pdf [4096], sample [4096, 3], is_w, is_i [4096, 3], is_pdf"""
    return _oracle_group(spec, block, params, "evalp_is" if name.startswith("is_") else name)[name]


def expected(spec, block, params, op):
    return tuple(oracle_output(spec, block, params, name) for name in OPS[op])


def host_outputs(b, block, params, op):
    """the product's object `b` (any context) on a block of host arrays, outputs as in OPS"""
    i, o, u1, u2 = BLOCKS[block]()
    up = mk_params(params) if params is not None else None
    if op in ("eval", "evalp", "pdf"):
        return (np.asarray(getattr(b, op)(i, o, up)),)
    if op in ("eval_pdf0", "eval_pdf1"):
        return tuple(np.asarray(a) for a in b.eval_pdf(i, o, up, cos=op == "eval_pdf1"))
    if op == "sample":
        return (np.asarray(b.sample(u1, u2, o, up)),)
    return tuple(np.asarray(a) for a in b.evalp_is(u1, u2, o, up))


def assert_second_trip_is_not_vacuous(tag, want, queued=None):
    """the units of the last, ragged trip (the block's first 4096 - 179) hold non-zero values -- and queued lanes"""
    m = BLOCK_N - RAGGED
    for a in want:
        with np.errstate(invalid="ignore"):
            live = int(np.count_nonzero(value_bits(a[:m]) & np.uint32(0x7fffffff)))
        assert live >= m // 16, f"{tag}: only {live} non-zero values in the last trip's {m} units"
    if queued is not None:
        assert int(queued[:m].sum()) >= 64, f"{tag}: {int(queued[:m].sum())} queued lanes in the last trip"


# ------------------------------------------------------------------ the capped kinds: (spec, block, parameter sets, trip family of eval, of sample)
CAPPED = {
    "tabular": ("tabular", "hostile", (None, ("elliptic", 0.2, 0.5, 0.7)), "capped", "capped"),
    "aniso": ("aniso", "hostile", (None,), "aniso_eval", "capped"),
    "sgd": ("sgd", "hostile", (None,), "capped", "capped"),
    "abc": ("abc", "hostile", (None,), "capped", "capped"),
    "lambert": ("lambert", "hostile", (None,), "capped", "capped"),
    "merl_exact": ("merl", "finite", (None,), "capped", "capped"),
    "utia_exact": ("utia", "finite", (None,), "capped", "capped"),
}

# the ten objects of tests/test_gpu_bounds.py (_objects) with its parameter sets: (spec, block, params)
BATCH_OBJECTS = {
    "ggx": (("mf", "ggx", FRESNEL_SCHLICK, True), "hostile", ("elliptic", 0.2, 0.5, 0.7)),
    "beckmann": (("mf", "beckmann", FRESNEL_IDEAL, True), "hostile", ("elliptic", 0.2, 0.5, 0.7)),
    "beckmann_sharp": (("mf", "beckmann", FRESNEL_UNPOLARIZED, False), "hostile", ("elliptic", 0.05, 0.05, 0.0)),
    "merl": ("merl", "finite", None), "utia": ("utia", "finite", None), "lambert": ("lambert", "hostile", None),
    "sgd": ("sgd", "hostile", None), "abc": ("abc", "hostile", None),
    "tabular": ("tabular", "hostile", ("elliptic", 0.4, 0.4, 0.0)), "aniso": ("aniso", "hostile", None),
}


# ------------------------------------------------------------------ device arrays between sentinels, and the calls through the C ABI
SENT_BITS = 0x7FC0DEAD          # a NaN no kernel produces (tests/test_gpu_bounds.py)
NAN_BITS = 0x7FC00000


def bits_i32(a):
    """value_bits as int32 (what a device tensor can hold)"""
    return value_bits(a).view(np.int32)


class Arr:
    """n units of `width` floats inside a flat device allocation prefilled with the sentinel.
    layout: "dense" -- `width` planes, each followed by at least one unit of sentinel and starting 16-byte aligned when `off` is a multiple of 4;
            "aos3" / "aos4" -- records of 3 / 4 floats (the fourth stays sentinel).  off: floats before the first unit (misalignment).  A scalar array
            (width 1) is one dense plane."""

    def __init__(self, torch, dev, n, width=3, layout="dense", off=0, data=None):
        self.torch, self.n, self.width, self.off = torch, n, width, off
        if width == 1 or layout == "dense":
            self.stride, self.plane = 1, (n + 1 + 3) // 4 * 4
            total = off + width * self.plane
        else:
            self.stride, self.plane = int(layout[3]), 1
            total = off + self.stride * (n + 1)
        self.t = torch.empty(total, dtype=torch.float32, device=dev)
        self.bits = self.t.view(torch.int32)
        self.bits.fill_(SENT_BITS)
        if data is not None:
            data = data.reshape(n, width)
            for c in range(width):
                self.comp(self.t, c).copy_(data[:, c])

    def comp(self, flat, c):
        first = self.off + c * self.plane
        return flat[first:first + self.stride * (self.n - 1) + 1:self.stride]

    def ptr(self, c=0):
        return self.t.data_ptr() + 4 * (self.off + c * self.plane)

    def view(self):
        v = _lib.Vec3View()
        v.x, v.y, v.z, v.stride = self.ptr(0), self.ptr(1), self.ptr(2), self.stride
        return v

    def values_bits(self):
        """[n, width] int32: the bits of every unit, NaNs as one pattern"""
        t = self.torch
        raw = t.stack([self.comp(self.bits, c) for c in range(self.width)], 1)
        val = t.stack([self.comp(self.t, c) for c in range(self.width)], 1)
        return raw, t.where(t.isnan(val), t.full_like(raw, NAN_BITS), raw)

    def values(self):
        out = self.torch.stack([self.comp(self.t, c) for c in range(self.width)], 1).cpu().numpy()
        return out[:, 0] if self.width == 1 else out

    def check_frame(self, tag, written=True):
        """nothing outside the n units was written; with `written`, every unit was"""
        t = self.torch
        sent = SENT_BITS
        raw, _ = self.values_bits()
        if written:
            left = int((raw == sent).sum())
            assert left == 0, f"{tag}: {left} output values were never written"
        rest = self.bits.clone()
        for c in range(self.width):
            self.comp(rest, c).fill_(sent)
        touched = int((rest != sent).sum())
        assert touched == 0, f"{tag}: {touched} values outside the output were written"

    def check_bits(self, tag, want_bits):
        """want_bits: [n, width] int32 device tensor (bits_i32 of the expected values)"""
        self.check_frame(tag)
        _, got = self.values_bits()
        bad = got != want_bits.reshape(self.n, self.width)
        nbad = int(bad.sum())
        if nbad:
            rows = self.torch.nonzero(bad.any(1)).reshape(-1)
            first = int(rows[0])
            g = got[first].cpu().numpy().view(np.float32); w = want_bits.reshape(self.n, self.width)[first].cpu().numpy().view(np.float32)
            where = [(int(r) // 1, (int(r) % BLOCK_N) // 64, int(r) % 64) for r in rows[:8].cpu().numpy()]
            raise AssertionError(f"{tag}: {nbad} of {bad.numel()} values differ from the oracle's bits in {int(rows.numel())} units; first at unit {first}: got {g} "
                                 f"want {w}; (unit, wave of the block, lane) of the first: {where}")


def device_of(ctx):
    """the torch device of a context's arrays (the host context: "cpu" -- the same calls then run the product's host path)"""
    return "cpu" if ctx.is_cpu else f"cuda:{ctx.device}"


def upload(torch, dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)           # a copy: the cases are read-only


def tile_dev(t, n):
    """a device block [4096, ...] repeated and cut to n units"""
    reps = -(-n // t.shape[0])
    return (t.repeat((reps,) + (1,) * (t.dim() - 1)) if reps > 1 else t)[:n]


def call(ctx, b, op, n, src, params, torch, dev, layouts=None, offs=None, rng=None):
    """One batch call through the C ABI on device memory.  src: {"i", "o", "u1", "u2"} -> device tensors [n, 3] / [n].  layouts / offs: per array name
    ("i", "o", "u1", "u2", "out", "pdf", "w") the vec3 layout and the float offset.  rng: (seed_u1, seed_u2, start) for sample_rng.
    Returns (inputs as Arr, outputs as Arr in the order of OPS[op])."""
    lib = _lib.load()
    layouts, offs = layouts or {}, offs or {}
    mk = lambda name, width, data=None: Arr(torch, dev, n, width, layouts.get(name, "dense"), offs.get(name, 0), data)
    pp = C.byref(params._p) if params is not None else None
    cx, h, nn, dm = ctx._h, b._h, C.c_int64(n), C.c_int(_lib.MEM_HOST if ctx.is_cpu else _lib.MEM_DEVICE)
    ins = {}
    if op in EVAL_OPS:
        ins["i"], ins["o"] = mk("i", 3, src["i"]), mk("o", 3, src["o"])
        vi, vo = ins["i"].view(), ins["o"].view()
        if op in ("eval", "evalp"):
            out = mk("out", 3); vout = out.view()
            _lib.check(getattr(lib, f"djb_{op}_batch")(cx, h, nn, C.byref(vi), C.byref(vo), pp, C.byref(vout), dm))
            outs = (out,)
        elif op == "pdf":
            pdf = mk("pdf", 1)
            _lib.check(lib.djb_pdf_batch(cx, h, nn, C.byref(vi), C.byref(vo), pp, C.c_void_p(pdf.ptr()), dm))
            outs = (pdf,)
        else:
            out, pdf = mk("out", 3), mk("pdf", 1); vout = out.view()
            _lib.check(lib.djb_eval_pdf_batch(cx, h, nn, C.byref(vi), C.byref(vo), pp, C.c_int(int(op[-1])), C.byref(vout), C.c_void_p(pdf.ptr()), dm))
            outs = (out, pdf)
    else:
        ins["o"] = mk("o", 3, src["o"]); vo = ins["o"].view()
        if rng is None:
            ins["u1"], ins["u2"] = mk("u1", 1, src["u1"]), mk("u2", 1, src["u2"])
        if op == "sample" and rng is not None:
            out = mk("out", 3); vout = out.view()
            _lib.check(lib.djb_sample_rng_batch(cx, h, nn, C.c_uint32(rng[0]), C.c_uint32(rng[1]), C.c_uint64(rng[2]), C.byref(vo), pp, C.byref(vout)))
            outs = (out,)
        elif op == "sample":
            out = mk("out", 3); vout = out.view()
            _lib.check(lib.djb_sample_batch(cx, h, nn, C.c_void_p(ins["u1"].ptr()), C.c_void_p(ins["u2"].ptr()), C.byref(vo), pp, C.byref(vout), dm))
            outs = (out,)
        else:
            w, out, pdf = mk("w", 3), mk("out", 3), mk("pdf", 1); vw, vout = w.view(), out.view()
            _lib.check(lib.djb_evalp_is_batch(cx, h, nn, C.c_void_p(ins["u1"].ptr()), C.c_void_p(ins["u2"].ptr()), C.byref(vo), pp, C.byref(vw), C.byref(vout),
                                              C.c_void_p(pdf.ptr()), dm))
            outs = (w, out, pdf)
    ctx.synchronize()
    return ins, outs


def check_inputs_unchanged(tag, ins, src):
    for name, a in ins.items():
        a.check_frame(f"{tag}: input {name}", written=False)
        assert bool((a.values_bits()[0] == src[name].reshape(a.n, a.width).view(a.torch.int32)).all()), f"{tag}: input {name} was modified"


# ------------------------------------------------------------------ every (object, block, parameter set, operators) the GPU modules compare
SAMPLER_SPECS = (("mf", "beckmann", FRESNEL_IDEAL, True), ("mf", "beckmann", FRESNEL_SCHLICK, True))
GGX_CONTRACT_SAMPLER = ("mf", "ggx", FRESNEL_IDEAL, True)
FIXUP = ((("mf", "ggx", FRESNEL_SCHLICK, True), ("elliptic", 0.3, 0.3, 0.0)), ("sgd", None))       # contract mode, worklist cap 0: evalp


def all_cases():
    """[(spec, block, params, operators)], without repeats"""
    out = []
    for f, s in SHARP_SETUPS:
        out += [(("mf", "beckmann", f, s), "sharp", p, EVAL_OPS) for p in SHARP_LOBES]
    for spec in SAMPLER_SPECS:
        out += [(spec, "sampler", p, SAMPLE_OPS) for p in SAMPLER_PARAMS]
    out += [(GGX_CONTRACT_SAMPLER, "sampler", p, ("sample",)) for p in SAMPLER_PARAMS]
    for spec, block, plist, _, _ in CAPPED.values():
        out += [(spec, block, p, EVAL_OPS + SAMPLE_OPS) for p in plist]
    out.append(("utia_drawn", "finite", None, ("eval", "evalp")))
    out += [(spec, "hostile", p, ("evalp",)) for spec, p in FIXUP]
    out += [(spec, block, p, EVAL_OPS + SAMPLE_OPS) for spec, block, p in BATCH_OBJECTS.values()]
    seen, uniq = set(), []
    for c in out:
        if c[:3] not in seen:
            seen.add(c[:3]); uniq.append(c)
    return uniq


def case_id(c):
    spec, block, p = c[:3]
    s = spec if isinstance(spec, str) else "-".join((spec[1], spec[2][0], "shadow" if spec[3] else "noshadow"))
    return f"{s}/{block}/" + ("default" if p is None else "_".join("%g" % v for v in p[1:]))
