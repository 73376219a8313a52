"""MERL material sets on the GPU (djb_kernels_merl_set.hip: one launch per batch): eval / evalp and proxy importance sampling of hits on
M resident tables against the oracle's per-material results selected by id (tests/merl_set_cases.py) -- bits equal in host, dense
and strided layouts and at the sizes where a tile bound can go wrong -- the exact-index fall-back, addressing beyond 2^32 bytes, output
bounds, the side check, graph capture, and objects of other contexts.

Figures: the eval kernel has no four-per-lane path, so there is no size threshold to straddle."""
import ctypes as C

import numpy as np
import pytest

import hit_calls
import merl_set_cases as cases
import proxy_is_cases
from dj_brdf_amd import _lib, djb, synth

pytestmark = pytest.mark.gpu
PREFIXES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025)
LAYOUTS = ("host", "dense", "strided")


@pytest.fixture(scope="module")
def mset(gpu_ctx):
    """the three-material set; its sources are destroyed before the first call"""
    members = cases.product_members(gpu_ctx)
    s = djb.merl_set(members, cases.product_params(), ctx=gpu_ctx)
    for b in members:
        b.close()
    yield s
    s.close()


@pytest.fixture(scope="module")
def proxies(gpu_ctx):
    return {"ggx": djb.ggx(ctx=gpu_ctx), "beckmann": djb.beckmann(ctx=gpu_ctx)}


def _vec(a, layout, dev):
    import torch
    return torch.from_numpy(np.array(a if layout == "strided" else a.T, order="C")).to(dev)        # [n, 3] | [3, n]


def _back(t, layout):
    a = t.cpu().numpy()
    return a if layout == "strided" else a.T


def _soa(t):
    """the view of a [3, n] device tensor, spelled out: djb._Vec reads a [3, 3] array as three records"""
    return hit_calls.view(t.data_ptr(), t.shape[1], "dense")


def _eval(s, ids, i, o, want_cos, layout):
    import torch
    call = s.evalp if want_cos else s.eval
    if layout == "host":
        return call(ids, i, o)
    dev = hit_calls.dev(s.ctx)
    dids = torch.from_numpy(np.array(ids)).to(dev)
    if layout == "strided":
        out = call(dids, _vec(i, layout, dev), _vec(o, layout, dev))
    else:
        n = len(ids)
        di, do, out = _vec(i, layout, dev), _vec(o, layout, dev), torch.empty((3, len(ids)), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().djb_merl_set_eval_batch(s.ctx._h, s._h, C.c_int64(n), C.c_void_p(dids.data_ptr()), C.byref(_soa(di)), C.byref(_soa(do)),
                                                      C.c_int(want_cos), C.byref(_soa(out)), C.c_int(_lib.MEM_DEVICE)))
    torch.cuda.synchronize()
    return _back(out, layout)


def _sample(s, proxy, ids, u1, u2, o, layout):
    import torch
    if layout == "host":
        return s.evalp_is_proxy(proxy, ids, u1, u2, o)
    dev = hit_calls.dev(s.ctx)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    dids, d1, d2, do = t(ids), t(u1), t(u2), _vec(o, layout, dev)
    if layout == "strided":
        w, i, pdf = s.evalp_is_proxy(proxy, dids, d1, d2, do)
    else:
        n = len(ids)
        w, i = (torch.empty((3, n), dtype=torch.float32, device=dev) for _ in range(2))
        pdf = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().djb_merl_set_evalp_is_proxy_batch(s.ctx._h, s._h, proxy._h, C.c_int64(n), C.c_void_p(dids.data_ptr()), C.c_void_p(d1.data_ptr()),
                                                                C.c_void_p(d2.data_ptr()), C.byref(_soa(do)), C.byref(_soa(w)), C.byref(_soa(i)),
                                                                C.c_void_p(pdf.data_ptr()), C.c_int(_lib.MEM_DEVICE)))
    torch.cuda.synchronize()
    return _back(w, layout), _back(i, layout), pdf.cpu().numpy()


def _assert_eval(tag, got, want):
    ok = cases.same_bits(got, want)
    assert got.shape == want.shape and ok.all(), f"{tag}: {int((~ok).sum())} of {ok.size} values differ, first at {tuple(np.argwhere(~ok)[0])}"


# ------------------------------------------------------------------ 1. both calls equal the oracle selection
@pytest.mark.parametrize("want_cos", [0, 1])
def test_eval_equals_the_oracle_selection(mset, want_cos):
    ids, bulk = cases.material_ids()
    cases.assert_ids_cover_every_class(ids, bulk)
    i, o = cases.eval_inputs()
    want = cases.expected_eval("evalp" if want_cos else "eval")
    for layout in LAYOUTS:
        _assert_eval(f"{layout}, n = {cases.N}", _eval(mset, ids, i, o, want_cos, layout), want)
    for n in PREFIXES:                     # units are independent: a prefix has the prefix's results
        for layout in ("dense", "strided"):
            _assert_eval(f"{layout}, n = {n}", _eval(mset, ids[:n], i[:n], o[:n], want_cos, layout), want[:n])


@pytest.mark.parametrize("proxy", ["ggx", "beckmann"])
def test_sampling_equals_the_oracle_selection(mset, proxies, proxy):
    ids, bulk = cases.material_ids()
    cases.assert_ids_cover_every_class(ids, bulk)
    o, u1, u2 = cases.sampler_inputs()
    want = cases.expected_sample(proxy)
    for layout in LAYOUTS:
        cases.assert_same(f"set <- {proxy}, {layout}, n = {cases.N}", _sample(mset, proxies[proxy], ids, u1, u2, o, layout), want)
    for n in PREFIXES:
        for layout in ("dense", "strided"):
            cases.assert_same(f"set <- {proxy}, {layout}, n = {n}", _sample(mset, proxies[proxy], ids[:n], u1[:n], u2[:n], o[:n], layout), [a[:n] for a in want])


# ------------------------------------------------------------------ 2. the fall-back is reached
def _near_normal_block(n):
    """o within 1e-3 rad of the normal, a quarter of them exactly on it, and a bulk of ordinary directions behind"""
    rng = np.random.default_rng(11)
    o = synth.directions_aos(n, synth.SEED_O).copy()
    m = n // 2
    t = rng.random(m) * 1e-3; ph = rng.random(m) * 6.2831853
    t[: m // 4] = 0
    o[:m] = np.stack([np.sin(t) * np.cos(ph), np.sin(t) * np.sin(ph), np.cos(t)], 1).astype(np.float32)
    return o, synth.uniforms(n, synth.SEED_U1), synth.uniforms(n, synth.SEED_U2)


def _guard_stats(ctx, i, o):
    import torch
    dev = hit_calls.dev(ctx)
    return djb.merl_guard_stats(torch.from_numpy(np.ascontiguousarray(i.T)).to(dev), torch.from_numpy(np.ascontiguousarray(o.T)).to(dev), ctx=ctx)


def test_pairs_that_tier_one_declines(gpu_ctx, mset, proxies, oracle):
    ids, _ = cases.material_ids()
    i, o = cases.eval_inputs()
    stats = _guard_stats(gpu_ctx, i, o)
    print("merl_guard_stats on the eval inputs:", stats)
    assert stats["ambiguous"] + stats["special"] > 0 and stats["certain"] > 0, stats
    # the sharp lobe of material 2 seen from next to the normal: h and d in and around the reference's snap zones
    n = cases.N
    so, su1, su2 = _near_normal_block(n)
    sids = np.full(n, 2, np.int32); sids[::53] = -1
    per = proxy_is_cases.compose(oracle, cases.oracle_materials()[2], oracle.microfacet("ggx"), cases.ORACLE_PARAMS[2], su1, su2, so)
    live = per[1][:, 2] > 0
    stats = _guard_stats(gpu_ctx, per[1][live], so[live])
    print("merl_guard_stats on the sampled pairs:", stats)
    assert stats["ambiguous"] + stats["special"] > 0 and stats["certain"] > 0, stats
    swant = [np.where((sids == 2)[:, None] if a.ndim == 2 else sids == 2, a, np.float32(0)) for a in per]
    want_eval = {c: cases.expected_eval("evalp" if c else "eval") for c in (0, 1)}
    for exact in (False, True):
        djb.set_merl_exact_only(gpu_ctx, exact)
        try:
            for layout in ("dense", "strided") + (() if exact else ("host",)):
                tag = f"{layout}, exact only = {exact}"
                cases.assert_same("sharp ggx, " + tag, _sample(mset, proxies["ggx"], sids, su1, su2, so, layout), swant)
                for c in (0, 1):
                    _assert_eval(f"eval cos = {c}, " + tag, _eval(mset, ids, i, o, c, layout), want_eval[c])
        finally:
            djb.set_merl_exact_only(gpu_ctx, False)


# ------------------------------------------------------------------ 3. addressing beyond 32 bits
def test_byte_offsets_beyond_two_to_the_32(gpu_ctx, proxies):
    """250 entries cycling the three tables: 4.4 GB, byte offsets across 2^31 (entry 123) and 2^32 (entry 246)"""
    import torch
    entries, n = 250, 4099
    members = cases.product_members(gpu_ctx)
    s = djb.merl_set([members[e % 3] for e in range(entries)], [cases.product_params()[e % 3] for e in range(entries)], ctx=gpu_ctx)
    try:
        for b in members:
            b.close()
        rng = np.random.default_rng(9)
        ids = rng.choice(np.int32([0, 1, 2, 122, 123, 124, 245, 246, 247, 249]), n).astype(np.int32)
        i, o = cases.eval_inputs()
        for c, op in ((0, "eval"), (1, "evalp")):
            want = cases.select([a[:n] for a in cases.eval_per_material(op)], ids % 3)
            for layout in ("dense", "strided", "host"):
                _assert_eval(f"250 entries, {op}, {layout}", _eval(s, ids, i[:n], o[:n], c, layout), want)
        so, u1, u2 = cases.sampler_inputs()
        per = cases.sample_per_material("ggx")
        want = tuple(cases.select([res[c][:n] for res in per], ids % 3) for c in range(3))
        for layout in ("dense", "strided"):
            cases.assert_same(f"250 entries, sampling, {layout}", _sample(s, proxies["ggx"], ids, u1[:n], u2[:n], so[:n], layout), want)
    finally:
        s.close()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 4. bounds
@pytest.mark.parametrize("layout", ["soa", "soa16", "aos"])
def test_outputs_stay_inside_their_bands(gpu_ctx, mset, proxies, layout):
    import torch
    from test_gpu_bounds import Buf
    lib = _lib.load()
    dev = hit_calls.dev(gpu_ctx)
    aos, a16 = layout == "aos", layout == "soa16"
    all_ids, _ = cases.material_ids()
    for n in (1, 3, 63, 65, 255, 257, 1023, 4097):
        hi, ho = synth.directions(n, 11), synth.directions(n, 12)              # [3, n]
        u1, u2 = synth.uniforms(n, 13), synth.uniforms(n, 14)
        ids = all_ids[2000:2000 + n] if n > 3 else np.int32([1, -1, 7][:n])
        mk = lambda planes=3, fill=None: Buf(torch, dev, n, planes, aos and planes == 3, fill, a16)
        bi, bo, bu1, bu2, bm = mk(fill=hi), mk(fill=ho), mk(1, [u1]), mk(1, [u2]), mk(1)
        bm.plane(0).view(torch.int32).copy_(torch.from_numpy(np.ascontiguousarray(ids)).to(dev))
        vi, vo = bi.view(), bo.view()
        tag = f"n={n} {layout}"
        for cos in (0, 1):
            out = mk(); vout = out.view()
            _lib.check(lib.djb_merl_set_eval_batch(gpu_ctx._h, mset._h, C.c_int64(n), C.c_void_p(bm.ptr()), C.byref(vi), C.byref(vo), C.c_int(cos),
                                                   C.byref(vout), C.c_int(_lib.MEM_DEVICE)))
            torch.cuda.synchronize(); out.check(tag + f" eval cos={cos}")
        for name, p in proxies.items():
            ow, oi, pdf = mk(), mk(), mk(1); vow, voi = ow.view(), oi.view()
            _lib.check(lib.djb_merl_set_evalp_is_proxy_batch(gpu_ctx._h, mset._h, p._h, C.c_int64(n), C.c_void_p(bm.ptr()), C.c_void_p(bu1.ptr()),
                                                             C.c_void_p(bu2.ptr()), C.byref(vo), C.byref(vow), C.byref(voi), C.c_void_p(pdf.ptr()),
                                                             C.c_int(_lib.MEM_DEVICE)))
            torch.cuda.synchronize()
            ow.check(tag + f" {name} (weight)"); oi.check(tag + f" {name} (i)"); pdf.check(tag + f" {name} (pdf)")
        for inp, what in ((bi, "i"), (bo, "o"), (bu1, "u1"), (bu2, "u2"), (bm, "material")):
            inp.check(tag + f" input {what}", written=False)
        assert np.array_equal(bm.plane(0).view(torch.int32).cpu().numpy(), ids), tag + ": the id array was modified"
        for k in range(3):
            assert np.array_equal(bi.plane(k).cpu().numpy().view(np.uint32), hi[k].view(np.uint32)), tag + ": i was modified"
            assert np.array_equal(bo.plane(k).cpu().numpy().view(np.uint32), ho[k].view(np.uint32)), tag + ": o was modified"
        assert np.array_equal(bu1.plane(0).cpu().numpy(), u1) and np.array_equal(bu2.plane(0).cpu().numpy(), u2), tag + ": a uniform was modified"


# ------------------------------------------------------------------ 5. the side check
def test_side_check_and_inactive_hits(gpu_ctx, proxies, oracle):
    """an active hit with i.z <= 0 follows the single-material rule -- i stored, weight 0, pdf 0 --, an inactive hit stores i = 0"""
    rng = np.random.default_rng(5)
    n = 4096
    z = np.concatenate([rng.random(3 * n // 4) * 0.05, -rng.random(n // 8) * 0.5, np.zeros(n // 8)]).astype(np.float32)
    ph = rng.random(n) * 6.2831853
    r = np.sqrt(1 - z.astype(np.float64) ** 2)
    o = np.stack([r * np.cos(ph), r * np.sin(ph), z], 1).astype(np.float32)
    u1, u2 = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
    ids = rng.integers(-1, cases.M + 1, n).astype(np.int32)
    rough = ("elliptic", 0.9, 0.9, 0.0)
    members = cases.product_members(gpu_ctx)
    s = djb.merl_set(members, [djb.microfacet.params.isotropic(0.9)] * cases.M, ctx=gpu_ctx)
    try:
        for name in ("ggx", "beckmann"):
            per = [proxy_is_cases.compose(oracle, om, oracle.microfacet(name), rough, u1, u2, o) for om in cases.oracle_materials()]
            want = tuple(cases.select([res[c] for res in per], ids) for c in range(3))
            for layout in LAYOUTS:
                got = _sample(s, proxies[name], ids, u1, u2, o, layout)
                cases.assert_same(f"rough {name}, {layout}", got, want)
            w, i, pdf = got
            act = cases.active(ids)
            side = act & (i[:, 2] <= 0)
            assert side.sum() > (30 if name == "ggx" else 0) and (act & (i[:, 2] > 0)).sum() > 100, int(side.sum())
            assert np.abs(i[side]).sum() > 0                                       # the direction is stored
            assert not w[side].view(np.uint32).any() and not pdf[side].view(np.uint32).any()
            assert (~act).sum() > 100 and not i[~act].view(np.uint32).any() and not w[~act].view(np.uint32).any() and not pdf[~act].view(np.uint32).any()
    finally:
        s.close()


# ------------------------------------------------------------------ 6. graph capture
def test_both_calls_replay_from_a_captured_graph(gpu_ctx, mset, proxies):
    import torch
    lib = _lib.load()
    n = 1 << 14
    dev = hit_calls.dev(gpu_ctx)
    i = djb.gen_directions(n, synth.SEED_I, ctx=gpu_ctx); o = djb.gen_directions(n, synth.SEED_O, ctx=gpu_ctx)
    u1 = djb.gen_uniforms(n, synth.SEED_U1, ctx=gpu_ctx); u2 = djb.gen_uniforms(n, synth.SEED_U2, ctx=gpu_ctx)
    ids = torch.from_numpy(np.ascontiguousarray(cases.material_ids()[0][:n])).to(dev)
    fr, w, si = (torch.zeros((3, n), dtype=torch.float32, device=dev) for _ in range(3))
    pdf = torch.zeros(n, dtype=torch.float32, device=dev)
    vi, vo, vfr, vw, vsi = djb._Vec(i), djb._Vec(o), djb._Vec(fr), djb._Vec(w), djb._Vec(si)

    def launch():
        _lib.check(lib.djb_merl_set_eval_batch(gpu_ctx._h, mset._h, C.c_int64(n), C.c_void_p(ids.data_ptr()), C.byref(vi.view), C.byref(vo.view),
                                               C.c_int(1), C.byref(vfr.view), C.c_int(_lib.MEM_DEVICE)))
        _lib.check(lib.djb_merl_set_evalp_is_proxy_batch(gpu_ctx._h, mset._h, proxies["beckmann"]._h, C.c_int64(n), C.c_void_p(ids.data_ptr()),
                                                         C.c_void_p(u1.data_ptr()), C.c_void_p(u2.data_ptr()), C.byref(vo.view), C.byref(vw.view),
                                                         C.byref(vsi.view), C.c_void_p(pdf.data_ptr()), C.c_int(_lib.MEM_DEVICE)))
    want, = hit_calls.graph_replay(gpu_ctx, launch, (fr, w, si, pdf), [lambda: None])      # one data set, resident
    assert want[0].abs().sum() > 0 and want[3].abs().sum() > 0


# ------------------------------------------------------------------ 7. contexts
def test_objects_of_other_contexts_are_refused(gpu_ctx, mset, proxies):
    import torch
    lib = _lib.load()
    n = 4096
    dev = hit_calls.dev(gpu_ctx)

    def status(ctx, s, proxy, mem_device):
        if mem_device:
            o = torch.zeros((3, n), dtype=torch.float32, device=dev); o[2] = 1
            u = torch.full((n,), 0.5, dtype=torch.float32, device=dev); ids = torch.zeros(n, dtype=torch.int32, device=dev)
            w, i, pdf = torch.zeros_like(o), torch.zeros_like(o), torch.zeros_like(u)
            ptr = lambda a: C.c_void_p(a.data_ptr())
        else:
            o = np.tile(np.float32([[0, 0, 1]]), (n, 1)); u = np.full(n, 0.5, np.float32); ids = np.zeros(n, np.int32)
            w, i, pdf = np.zeros_like(o), np.zeros_like(o), np.zeros_like(u)
            ptr = lambda a: C.c_void_p(a.ctypes.data)
        vo, vw, vi = djb._Vec(o), djb._Vec(w), djb._Vec(i)
        mem = C.c_int(_lib.MEM_DEVICE if mem_device else _lib.MEM_HOST)
        if proxy is None:
            st = lib.djb_merl_set_eval_batch(ctx._h, s._h, C.c_int64(n), ptr(ids), C.byref(vo.view), C.byref(vo.view), C.c_int(0), C.byref(vw.view), mem)
        else:
            st = lib.djb_merl_set_evalp_is_proxy_batch(ctx._h, s._h, proxy._h, C.c_int64(n), ptr(ids), ptr(u), ptr(u), C.byref(vo.view), C.byref(vw.view),
                                                       C.byref(vi.view), ptr(pdf), mem)
        return st, lib.djb_last_error().decode(errors="replace")

    other = djb.Context(gpu_ctx.device)
    cpu = djb.cpu_context()
    cpu_members = cases.product_members(cpu)[:1]
    cpu_set = djb.merl_set(cpu_members, [djb.microfacet.params.isotropic(0.3)], ctx=cpu)
    try:
        for mem_device in (False, True):
            st, msg = status(gpu_ctx, mset, djb.ggx(ctx=other), mem_device)
            assert st == 1 and "different contexts" in msg, (st, msg)
            st, msg = status(other, mset, None, mem_device)
            assert st == 1 and "another context" in msg, (st, msg)
            st, msg = status(gpu_ctx, mset, djb.tabular(djb.ggx(ctx=gpu_ctx), 16, True, ctx=gpu_ctx), mem_device)
            assert st == 5 and "ggx or beckmann" in msg, (st, msg)
        for proxy in (None, proxies["ggx"]):
            st, msg = status(gpu_ctx, cpu_set, proxy, False)
            assert st == 1 and "different back ends" in msg, (st, msg)
        st, msg = status(cpu, mset, None, False)
        assert st == 1 and "different back ends" in msg, (st, msg)
        # a member of another context, at creation
        foreign = djb.merl.from_table(cases.tables()[1], ctx=other)
        ptrs = (C.c_void_p * 1)(foreign._h.value)
        out = C.c_void_p()
        st = lib.djb_merl_set_create(gpu_ctx._h, C.c_int(1), ptrs, None, C.byref(out))
        assert st == 1 and "another context" in lib.djb_last_error().decode(errors="replace")
        st, msg = status(gpu_ctx, mset, proxies["ggx"], True)
        assert st == 0, msg
        torch.cuda.synchronize()
    finally:
        cpu_set.close()
