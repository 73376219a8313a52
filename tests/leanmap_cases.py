"""Shared by tests/test_leanmap_host.py (CPU context) and tests/test_gpu_leanmap.py (MI355X): the numpy float32 restatement of
the LEAN-map definition of include/djb_hip.h (level 0 of utils/nmap2leanmap.cpp, the pyramid, the trilinear lookup) and the
checks both back ends must pass.  Every numpy expression below performs one float32 operation per step, in the order the header
gives, so results are compared for EQUAL BITS.  The one allowance: where the definition produces a NaN (inf - inf, inf * 0 in a map
that holds infinite moments) the NaN's sign / payload is the hardware's (x86 produces the negative quiet NaN, gfx950 the positive
one), so NaNs must sit in the same places and everything else must have the same bits."""
import ctypes as C
import os

import numpy as np

from dj_brdf_amd import _lib, djb, synth

f32 = np.float32
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAPS = ["n64x32", "n1x1", "n2x1", "n1x4", "b128x128"]
P = djb.microfacet.params


def fixture():
    return np.load(os.path.join(G, "leanmap.npz"))


def same(a, b):
    """equal bits; NaNs in the same places (see the module docstring)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def first_diff(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    bad = np.argwhere(~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    return f"{len(bad)} differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}" if len(bad) else "equal"


def to_np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


# ------------------------------------------------------------------ the definition, in numpy float32
def nmap2leanmap_np(nmap, base_roughness):
    """utils/nmap2leanmap.cpp:33-54 -> [h, w, 5] = E1..E5"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t1 = (nmap[..., 0].astype(f32) / f32(255)) * f32(2) - f32(1)
        t2 = (nmap[..., 1].astype(f32) / f32(255)) * f32(2) - f32(1)
        t3 = nmap[..., 2].astype(f32) / f32(255)
        sx, sy = -t1 / t3, -t2 / t3
        br = f32(0.5) * f32(base_roughness) * f32(base_roughness)
        return np.stack([sx, sy, sx * sx + br, sy * sy + br, sx * sy], 2).astype(f32)


def pyramid_np(level0):
    levels = [np.ascontiguousarray(level0, f32)]
    with np.errstate(invalid="ignore", over="ignore"):
        while levels[-1].shape[0] > 1 or levels[-1].shape[1] > 1:
            T = levels[-1]
            hs, ws = T.shape[:2]
            x, y = np.arange(max(1, ws // 2)), np.arange(max(1, hs // 2))
            x0, x1 = np.minimum(2 * x, ws - 1), np.minimum(2 * x + 1, ws - 1)
            y0, y1 = np.minimum(2 * y, hs - 1), np.minimum(2 * y + 1, hs - 1)
            levels.append(((T[y0][:, x0] + T[y0][:, x1]) + (T[y1][:, x0] + T[y1][:, x1])) * f32(0.25))
    return levels


def _frac(u):
    with np.errstate(invalid="ignore"):
        f = u - np.floor(u)
        return np.where((f >= 0) & (f < 1), f, f32(0)).astype(f32)


def _lerp(a, b, s):
    return a + (b - a) * s


def _bilinear(T, uf, vf):
    h, w = T.shape[:2]
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = uf * f32(w) - f32(0.5), vf * f32(h) - f32(0.5)
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = (x - x0)[:, None], (y - y0)[:, None]
        c0, r0 = x0.astype(np.int64) % w, y0.astype(np.int64) % h                   # repeat
        c1, r1 = (x0.astype(np.int64) + 1) % w, (y0.astype(np.int64) + 1) % h
        return _lerp(_lerp(T[r0, c0], T[r0, c1], fx), _lerp(T[r1, c0], T[r1, c1], fx), fy)


def lookup_np(levels, uv, lod=None):
    uv = np.ascontiguousarray(uv, f32)
    n, top = len(uv), len(levels) - 1
    lod = np.zeros(n, f32) if lod is None else np.array(lod, f32)
    lod[np.isnan(lod)] = 0
    lod = np.where(lod < 0, f32(0), np.where(lod > f32(top), f32(top), lod)).astype(f32)
    lf = np.floor(lod)
    l0, t = lf.astype(np.int64), (lod - lf).astype(f32)
    l1 = np.minimum(l0 + 1, top)
    uf, vf = _frac(uv[:, 0]), _frac(uv[:, 1])
    out = np.empty((n, 5), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(top + 1):
            s = l0 == l
            if s.any():
                out[s] = _bilinear(levels[l], uf[s], vf[s])
        for l in range(top + 1):
            s = (l1 == l) & (t != 0)
            if s.any():
                b = _bilinear(levels[l], uf[s], vf[s])
                out[s] = _lerp(out[s], b, t[s][:, None])
    return out


def hostile_coords(n, levels, seed):
    """(uv, lod): random coordinates inside and far outside [0, 1), lods below 0, above the top, integral, NaN; u = NaN / inf"""
    rng = np.random.default_rng(seed)
    uv = (rng.random((n, 2)) * 6 - 3).astype(f32)
    lod = (rng.random(n) * (levels + 2) - 1).astype(f32)
    k = np.arange(n)
    lod[k % 7 == 0] = np.floor(lod[k % 7 == 0])
    lod[k % 101 == 3] = np.nan
    lod[k % 103 == 5] = np.inf
    lod[k % 107 == 5] = -np.inf
    uv[k % 109 == 1, 0] = np.nan
    uv[k % 113 == 2, 1] = np.inf
    uv[k % 127 == 3, 0] = -np.inf
    uv[k % 131 == 4, 0] = -1e-9            # the fraction rounds up to 1
    uv[k % 137 == 6, 1] = 1e30
    uv[k % 139 == 7] = (rng.integers(-4, 5, (len(uv[k % 139 == 7]), 2))).astype(f32)      # exact integers
    return uv, lod


def all_maps(ctx):
    """[(name, map object, numpy level 0)] for every fixture map, built from the fixture's reference normal map (scale 0.1)"""
    g = fixture()
    out = []
    for name in MAPS:
        nmap = g[f"nmap_{name}_s01"]
        out.append((name, djb.leanmap.from_nmap(nmap, 1e-5, ctx=ctx), nmap2leanmap_np(nmap, 1e-5)))
    out.append(("hostile", djb.leanmap.from_nmap(g["nmap_hostile"], 0.05, ctx=ctx), g["lean_hostile"]))
    return out


# ------------------------------------------------------------------ checks both back ends run
def check_level0_against_reference(ctx):
    """item 1: dmap -> nmap bytes of the compiled reference at two scales; level 0 == the recorded moments; from_dmap == the chain"""
    g = fixture()
    for name in MAPS:
        d = g[f"dmap_{name}"]
        for tag, scale in (("s01", 0.1), ("s4", 4.0)):
            got = djb.dmap_to_nmap(d, scale, ctx=ctx)
            assert np.array_equal(got, g[f"nmap_{name}_{tag}"]), (name, scale, int((got != g[f"nmap_{name}_{tag}"]).sum()))
        nmap = g[f"nmap_{name}_s01"]
        want = g[f"lean_{name}_s01"] if f"lean_{name}_s01" in g.files else nmap2leanmap_np(nmap, 1e-5)
        m = djb.leanmap.from_nmap(nmap, 1e-5, ctx=ctx)
        assert (m.width, m.height) == (d.shape[1], d.shape[0]) and m.levels == 1 + max(d.shape).bit_length() - 1
        assert same(m.level(0), want), (name, first_diff(m.level(0), want))
        rgba = np.concatenate([nmap, np.full(nmap.shape[:2] + (1,), 255, np.uint8)], 2)         # pixel_stride 4
        assert same(djb.leanmap.from_nmap(rgba, 1e-5, ctx=ctx).level(0), want), name
        for scale, tag in ((0.1, "s01"), (4.0, "s4")):
            md = djb.leanmap.from_dmap(d, scale, 1e-5, ctx=ctx)
            assert same(md.level(0), nmap2leanmap_np(g[f"nmap_{name}_{tag}"], 1e-5)), (name, scale)
    # blue bytes of 0 and 1: the reference's infinities, not a clamp
    m = djb.leanmap.from_nmap(g["nmap_hostile"], 0.05, ctx=ctx)
    l0 = m.level(0)
    assert same(l0, g["lean_hostile"]), first_diff(l0, g["lean_hostile"])
    assert np.isinf(l0[0, 0, :2]).all() and np.isinf(l0[3, 7, 0]) and np.isfinite(l0[2, 5]).all()


def check_moments_import_and_bias(ctx):
    """create_from_moments (plain and from the _biased tool) and get_level(biased=1)"""
    g = fixture()
    l0 = nmap2leanmap_np(g["nmap_n64x32_s01"], 1e-5)
    m = djb.leanmap.from_moments(l0, ctx=ctx)
    assert same(m.level(0), l0)
    bias = np.array([25, 25, 0, 0, 625], f32)
    biased = (l0 + bias).astype(f32)                                    # what nmap2leanmap_biased stores
    assert same(m.level(0, biased=True), biased)
    mb = djb.leanmap.from_moments(biased, biased=True, ctx=ctx)
    assert same(mb.level(0), (biased - bias).astype(f32))
    ref = pyramid_np(l0)
    for l in range(m.levels):
        assert same(m.level(l, biased=True), (ref[l] + bias).astype(f32)), l


def check_pyramid_and_lookup(ctx, n=100_000, device=None):
    """item 2: every level of every fixture map, >= 1e5 hostile lookups per map family, and the closed-form cases"""
    for name, m, l0 in all_maps(ctx):
        ref = pyramid_np(l0)
        assert m.levels == len(ref), name
        for l in range(m.levels):
            got = m.level(l)
            assert got.shape == ref[l].shape and same(got, ref[l]), (name, l, first_diff(got, ref[l]))
        uv, lod = hostile_coords(n if name in ("n64x32", "b128x128", "hostile") else 4096, m.levels, 11)
        want = lookup_np(ref, uv, lod)
        got = _lookup(m, uv, lod, device)
        assert same(got, want), (name, first_diff(got, want))
        assert same(_lookup(m, uv, None, device), lookup_np(ref, uv, None)), name      # lod == NULL: level 0
        if name == "hostile":
            continue
        h, w = l0.shape[:2]
        yy, xx = np.mgrid[0:h, 0:w]
        centres = np.stack([(xx.ravel() + 0.5) / w, (yy.ravel() + 0.5) / h], 1).astype(f32)
        got = _lookup(m, centres, np.zeros(len(centres), f32), device)
        assert same(got, l0.reshape(-1, 5)), (name, "texel centres")
        anywhere = hostile_coords(4096, m.levels, 5)[0]
        got = _lookup(m, anywhere, np.full(4096, m.levels - 1, f32), device)
        assert same(got, np.broadcast_to(ref[-1].reshape(1, 5), (4096, 5))), (name, "top level")


def _lookup(m, uv, lod, device):
    if device is None:
        return m.lookup(uv, lod)
    import torch
    r = m.lookup(torch.as_tensor(uv, device=device), None if lod is None else torch.as_tensor(lod, device=device))
    assert r.is_cuda
    return to_np(r)


def lobes(ctx):
    return [("beckmann", djb.beckmann(djb.fresnel.ideal(), True, ctx=ctx)),
            ("ggx", djb.ggx(djb.fresnel.schlick((1.0, 0.71, 0.29)), True, ctx=ctx))]


def check_fused_equals_composed(ctx, sizes, device=None):
    """item 3: eval_leanmap(uv, lod) == eval_lean(lookup(uv, lod)) and the same for sample: values and written-back parameters"""
    g = fixture()
    m = djb.leanmap.from_nmap(g["nmap_b128x128_s01"], 1e-5, ctx=ctx)
    base = P.elliptic(0.12, 0.2, 0.3)
    for n in sizes:
        i, o = synth.directions_aos(n, synth.SEED_I), synth.directions_aos(n, synth.SEED_O)
        u1, u2 = synth.uniforms(n, synth.SEED_U1), synth.uniforms(n, synth.SEED_U2)
        uv, lod = hostile_coords(n, m.levels, 23)
        if device is not None:
            import torch
            i, o, u1, u2, uv, lod = (torch.as_tensor(np.ascontiguousarray(a), device=device) for a in (i, o, u1, u2, uv, lod))
        rec = m.lookup(uv, lod)
        for lname, b in lobes(ctx):
            for filtering in (True, False):
                for scale in (1.0, 0.37):
                    for want in ("eval", "evalp", "pdf", "eval+pdf", "evalp+pdf"):
                        a = b.eval_leanmap(i, o, m, uv, lod, base, scale, want=want, return_params=True, filtering=filtering)
                        c = b.eval_lean(i, o, base, scale, rec, want=want, return_params=True, filtering=filtering)
                        for x, y in zip(a, c):
                            assert same(to_np(x), to_np(y)), (lname, n, filtering, scale, want, first_diff(to_np(x), to_np(y)))
                    for is_ in (True, False):
                        a = b.sample_leanmap(u1, u2, o, m, uv, lod, base, scale, evalp_is=is_, return_params=True, filtering=filtering)
                        c = b.sample_lean(u1, u2, o, base, scale, rec, evalp_is=is_, return_params=True, filtering=filtering)
                        for x, y in zip(a, c):
                            assert same(to_np(x), to_np(y)), (lname, n, filtering, scale, "sample", is_, first_diff(to_np(x), to_np(y)))
        # lod == None on the fused calls: level 0
        b = lobes(ctx)[0][1]
        a = b.eval_leanmap(i, o, m, uv, None, base, 1.0, want="evalp", return_params=True)
        c = b.eval_lean(i, o, base, 1.0, m.lookup(uv, None), want="evalp", return_params=True)
        assert all(same(to_np(x), to_np(y)) for x, y in zip(a, c))


def check_lean_property(ctx):
    """item 5: filtering the moments can only widen the lobe; the naive mip loses exactly that"""
    g = fixture()
    nmap = g["nmap_b128x128_s01"]
    l0 = nmap2leanmap_np(nmap, 1e-5).astype(np.float64)
    var = (l0[..., 2].mean() - l0[..., 0].mean() ** 2, l0[..., 3].mean() - l0[..., 1].mean() ** 2)
    assert min(var) >= 1e-2, var                     # far above float rounding of E3 (~1e-7 relative)
    m = djb.leanmap.from_nmap(nmap, 1e-5, ctx=ctx)
    h, w = nmap.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    uv = np.stack([(xx.ravel() + 0.5) / w, (yy.ravel() + 0.5) / h], 1).astype(f32)
    n = len(uv)
    i, o = synth.directions_aos(n, synth.SEED_I), synth.directions_aos(n, synth.SEED_O)
    b, base = djb.beckmann(ctx=ctx), P.isotropic(0.1)
    pp = lambda lod, filtering=True: b.eval_leanmap(i, o, m, uv, np.full(n, lod, f32), base, 1.0, want="evalp", return_params=True,
                                                    filtering=filtering)[1]
    fine, top, naive = pp(0), pp(m.levels - 1), pp(m.levels - 1, False)
    for c in (0, 1):                                 # ax, ay
        assert (top[:, c] >= fine[:, c]).all() and (top[:, c] > fine[:, c]).any(), c
        assert (naive[:, c] < top[:, c]).all(), c
    # a flat map: every level gives the parameters of level 0, at texel centres and anywhere else
    flat = djb.leanmap.from_nmap(np.broadcast_to(np.array([140, 120, 240], np.uint8), (16, 32, 3)), 1e-5, ctx=ctx)
    want = None
    for l in range(flat.levels):
        hl, wl = flat.level_shape(l)
        yy, xx = np.mgrid[0:hl, 0:wl]
        c = np.stack([(xx.ravel() + 0.5) / wl, (yy.ravel() + 0.5) / hl], 1).astype(f32)
        c = np.concatenate([c, hostile_coords(64, flat.levels, l)[0]])
        c = c[np.isfinite(c).all(1)]
        k = len(c)
        got = b.eval_leanmap(i[:k], o[:k], flat, c, np.full(k, l, f32), base, 1.0, want="evalp", return_params=True)[1]
        want = got[0] if want is None else want
        assert same(got, np.broadcast_to(want, got.shape)), l


def check_errors(ctx):
    """item 6 (the part one context can show): sizes, null pointers, DJB_LEAN_BIASED on a fused call, destroy twice / destroy NULL"""
    import pytest
    lib = _lib.load()
    ok = np.zeros((4, 4, 3), np.uint8) + 128
    for shape in ((3, 4), (4, 6), (0, 4), (4, 16384)):
        with pytest.raises(djb.exc) as e:
            djb.leanmap.from_nmap(np.zeros(shape + (3,), np.uint8), ctx=ctx)
        assert e.value.status == 1 and "2^a x 2^b" in str(e.value), str(e.value)
        with pytest.raises(djb.exc):
            djb.leanmap.from_dmap(np.zeros(shape, np.uint8), ctx=ctx)
        with pytest.raises(djb.exc):
            djb.leanmap.from_moments(np.zeros(shape + (5,), f32), ctx=ctx)
        with pytest.raises(djb.exc):
            djb.dmap_to_nmap(np.zeros(shape, np.uint8), ctx=ctx)
    h = C.c_void_p()
    assert lib.djb_leanmap_create_from_nmap(ctx._h, 4, 4, None, 3, C.c_float(0), C.byref(h)) == 1 and not h
    assert lib.djb_leanmap_create_from_nmap(ctx._h, 4, 4, C.c_void_p(ok.ctypes.data), 2, C.c_float(0), C.byref(h)) == 1 and not h
    assert lib.djb_leanmap_create_from_nmap(ctx._h, 4, 4, C.c_void_p(ok.ctypes.data), 3, C.c_float(0), None) == 1
    assert lib.djb_leanmap_create_from_nmap(None, 4, 4, C.c_void_p(ok.ctypes.data), 3, C.c_float(0), C.byref(h)) == 1
    assert lib.djb_leanmap_create_from_dmap(ctx._h, 4, 4, None, C.c_float(1), C.c_float(0), C.byref(h)) == 1
    assert lib.djb_leanmap_create_from_moments(ctx._h, 4, 4, None, 0, C.byref(h)) == 1
    assert lib.djb_dmap_to_nmap(ctx._h, 4, 4, None, C.c_float(1), C.c_void_p(ok.ctypes.data)) == 1
    assert lib.djb_leanmap_info(None, None, None, None) == 1
    m = djb.leanmap.from_nmap(ok, ctx=ctx)
    out = np.zeros((16, 5), f32)
    assert lib.djb_leanmap_get_level(m._h, 3, 0, C.c_void_p(out.ctypes.data)) == 1 and b"levels 0 .. 2" in lib.djb_last_error()
    assert lib.djb_leanmap_get_level(m._h, 0, 0, None) == 1
    uv = np.zeros((4, 2), f32)
    assert lib.djb_leanmap_lookup_batch(ctx._h, None, C.c_int64(4), C.c_void_p(uv.ctypes.data), None, C.c_void_p(out.ctypes.data), 1) == 1
    assert lib.djb_leanmap_lookup_batch(ctx._h, m._h, C.c_int64(4), None, None, C.c_void_p(out.ctypes.data), 1) == 1
    assert lib.djb_leanmap_lookup_batch(ctx._h, m._h, C.c_int64(4), C.c_void_p(uv.ctypes.data), None, None, 1) == 1
    # the fused calls: DJB_LEAN_BIASED (2) is an invalid argument, so is an unknown flag, a null map, a null uv
    b = djb.beckmann(ctx=ctx)
    i = np.ascontiguousarray(synth.directions_aos(4, 1), f32)
    vi, fr = djb._Vec(i), djb._Vec(np.zeros((4, 3), f32))
    base = P.isotropic(0.1)
    u = np.full(4, 0.5, f32)

    def ev(mp, uvp, flags):
        return lib.djb_eval_leanmap_batch(ctx._h, b._h, mp, C.c_int64(4), C.byref(vi.view), C.byref(vi.view), uvp, None, C.byref(base._p),
                                          C.c_float(1), flags, 2, C.byref(fr.view), None, None, 1)

    def sa(mp, uvp, flags):
        return lib.djb_sample_leanmap_batch(ctx._h, b._h, mp, C.c_int64(4), C.c_void_p(u.ctypes.data), C.c_void_p(u.ctypes.data), C.byref(vi.view),
                                            uvp, None, C.byref(base._p), C.c_float(1), flags, None, C.byref(fr.view), None, None, 1)
    uvp = C.c_void_p(uv.ctypes.data)
    for call in (ev, sa):
        assert call(m._h, uvp, 0) == 0, lib.djb_last_error()
        assert call(m._h, uvp, 1) == 0
        assert call(m._h, uvp, 2) == 1 and b"DJB_LEAN_BIASED" in lib.djb_last_error()
        assert call(m._h, uvp, 3) == 1
        assert call(m._h, uvp, 4) == 1 and b"unknown LEAN flag" in lib.djb_last_error()
        assert call(None, uvp, 0) == 1
        assert call(m._h, None, 0) == 1
    with pytest.raises(djb.exc):
        b.eval_leanmap(i, i, m, uv, None, base, -1.0)                # lrep::operator*= asserts sc >= 0
    with pytest.raises(djb.exc):
        djb.lambert(ctx=ctx).eval_leanmap(i, i, m, uv, None, base, 1.0) if hasattr(djb.lambert, "eval_leanmap") else \
            _lib.check(lib.djb_eval_leanmap_batch(ctx._h, djb.lambert(ctx=ctx)._h, m._h, C.c_int64(4), C.byref(vi.view), C.byref(vi.view), uvp, None,
                                                  C.byref(base._p), C.c_float(1), 0, 2, C.byref(fr.view), None, None, 1))
    m.close(); m.close()                                             # destroy twice through the wrapper: the handle is cleared
    assert lib.djb_leanmap_destroy(None) == 0


# ------------------------------------------------------------------ records a map produces, through the per-hit operators, against the oracle
STEEP_ROUGHNESS = (1e-5, 0.05)
LEAN_BASE_T = ("elliptic", 0.12, 0.2, 0.3)
LEAN_LOBES_T = [("beckmann", ("ideal",)), ("ggx", ("schlick", 1.0, 0.71, 0.29))]          # lobes(ctx), in the oracle's form
ZERO_VARIANCE_SHARE = 0.25


def steep_nmap(seed=41):
    """a 64 x 64 normal map of steep facets: red / green uniform over 0..255, blue uniform over 1..12 -- slopes up to 255, so that
    E3 = sx^2 + base_roughness^2 / 2 rounds to sx^2 at base_roughness = 1e-5 and a texel has NO variance left (E3 - E1^2 <= 0)"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 256, (64, 64)), rng.integers(0, 256, (64, 64)), rng.integers(1, 13, (64, 64))], 2).astype(np.uint8)


def steep_coords(n, levels, seed, w=64, h=64):
    """hostile_coords with every third hit at the centre of a level-0 texel (lod 0): records that ARE texels"""
    uv, lod = hostile_coords(n, levels, seed)
    rng = np.random.default_rng(seed + 1)
    k = np.arange(n) % 3 == 0
    m = int(k.sum())
    uv[k] = np.stack([(rng.integers(0, w, m) + 0.5) / w, (rng.integers(0, h, m) + 0.5) / h], 1).astype(f32)
    lod[k] = 0
    return uv, lod


def zero_variance_share(rec):
    """of the records with finite moments, the share whose slope variance in x is not positive (float32, as the definition computes it)"""
    rec = np.ascontiguousarray(rec, f32)
    fin = np.isfinite(rec).all(1)
    with np.errstate(over="ignore", invalid="ignore"):
        var = rec[fin, 2] - rec[fin, 0] * rec[fin, 0]
    return float(np.mean(var <= 0)) if fin.any() else 0.0


def check_map_records_against_oracle(ctx, oracle, n=6000, device=None):
    """For every fixture map, the hostile map (infinite moments) and a steep map (zero-variance texels) at two base roughnesses:
    rec = map.lookup(hostile coordinates: every level, filtered top levels, NaN / Inf coordinates), then
      eval_lean / sample_lean(rec)        == oracle.eval_lean / oracle.sample_lean on the same records: values and written-back pdfparams,
      eval_leanmap / sample_leanmap(uv, lod) == the same oracle output,
    with LEAN filtering on and off and dmapscale 1, 0.37 and 0.  Equal bits, NaNs in the same places (the module docstring)."""
    maps = [(name, m, l0, hostile_coords) for name, m, l0 in all_maps(ctx)]
    steep = steep_nmap()
    for br in STEEP_ROUGHNESS:
        l0 = nmap2leanmap_np(steep, br)
        maps.append((f"steep{br}", djb.leanmap.from_nmap(steep, br, ctx=ctx), l0, steep_coords))
    base = P.elliptic(*LEAN_BASE_T[1:])
    i, o = synth.directions_aos(n, synth.SEED_I), synth.directions_aos(n, synth.SEED_O)
    u1, u2 = synth.uniforms(n, synth.SEED_U1), synth.uniforms(n, synth.SEED_U2)
    if device is not None:
        import torch
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)
    else:
        dev = lambda a: a
    di, do, d1, d2 = dev(i), dev(o), dev(u1), dev(u2)
    for name, m, l0, coords in maps:
        uv, lod = coords(n, m.levels, 37)
        ref = lookup_np(pyramid_np(l0), uv, lod)
        if name == "steep1e-05":
            z = zero_variance_share(ref)                              # from the numpy restatement alone
            assert z >= ZERO_VARIANCE_SHARE, f"only {z:.3f} of the steep map's finite records have no variance left"
        if name == "hostile":
            assert not np.isfinite(ref).all()                         # infinite moments do reach the per-hit operators
        duv, dlod = dev(uv), dev(lod)
        drec = m.lookup(duv, dlod)
        rec = to_np(drec)
        assert same(rec, ref), (name, first_diff(rec, ref))
        for (lname, b), (oname, fres) in zip(lobes(ctx), LEAN_LOBES_T):
            assert lname == oname
            ob = oracle.microfacet(oname, fres, True)
            for filtering in (True, False):
                for scale in (1.0, 0.37, 0.0):
                    tag = (name, lname, filtering, scale)
                    for op in ("eval", "evalp", "pdf"):
                        want = oracle.eval_lean(ob, i, o, LEAN_BASE_T, scale, rec, op, filtering=filtering)
                        got = b.eval_lean(di, do, base, scale, drec, want=op, return_params=True, filtering=filtering)
                        fused = b.eval_leanmap(di, do, m, duv, dlod, base, scale, want=op, return_params=True, filtering=filtering)
                        for how, g in (("eval_lean", got), ("eval_leanmap", fused)):
                            for what, x, y in zip(("value", "pdfparams"), g, want):
                                assert same(to_np(x), y), (tag, op, how, what, first_diff(to_np(x), y))
                    for is_ in (True, False):
                        want = oracle.sample_lean(ob, u1, u2, o, LEAN_BASE_T, scale, rec, evalp_is=is_, filtering=filtering)
                        got = b.sample_lean(d1, d2, do, base, scale, drec, evalp_is=is_, return_params=True, filtering=filtering)
                        fused = b.sample_leanmap(d1, d2, do, m, duv, dlod, base, scale, evalp_is=is_, return_params=True, filtering=filtering)
                        for how, g in (("sample_lean", got), ("sample_leanmap", fused)):
                            assert len(g) == len(want)
                            for k, (x, y) in enumerate(zip(g, want)):
                                assert same(to_np(x), y), (tag, "evalp_is" if is_ else "sample", how, k, first_diff(to_np(x), y))
        m.close()
