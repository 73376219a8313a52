"""Proxy importance sampling on the GPU (djb_kernels_proxy.hip: one launch per batch): every pair of kinds against the operator's
definition composed from the oracle's separate operators (tests/proxy_is_cases.py) -- bits equal for weight, direction and pdf, in
host, dense and strided layouts, at the sizes where a tile bound or the host-twin boundary can go wrong -- the MERL fall-back, the
pairs the kernels do not serve, objects of two contexts, graph capture, and the contract option."""
import ctypes as C

import numpy as np
import pytest

import proxy_is_cases as cases
from dj_brdf_amd import _lib, djb
from hit_calls import graph_replay

pytestmark = pytest.mark.gpu
N = 150_001
DEVICE_SIZES = (1, 63, 64, 65, 255, 256, 257)        # around a wave and a 256-unit tile
HOST_SIZES = (96, 97)                                 # the host twin answers up to DJB_SCALAR_HOST_MAX = 96 units


@pytest.fixture(scope="module")
def objects(gpu_ctx):
    """the product's objects on the GPU context, built once"""
    cache = {}

    def get(role, name):
        key = (role, cases.PROXIES[name][0] if name in cases.PROXIES else name)
        if key not in cache:
            cache[key] = (cases.product_target if role == "target" else cases.product_proxy)(name, gpu_ctx)
        return cache[key]
    return get


def _run(target, proxy, params, u1, u2, o, layout, tparams=None):
    """one call in the given layout -> (weight [n,3], i [n,3], pdf [n]) as numpy"""
    import torch
    if layout == "host":
        return target.evalp_is_proxy(proxy, u1, u2, o, tparams, params)
    dev = f"cuda:{target.ctx.device}"
    d1, d2 = torch.from_numpy(np.ascontiguousarray(u1)).to(dev), torch.from_numpy(np.ascontiguousarray(u2)).to(dev)
    do = torch.from_numpy(np.ascontiguousarray(o if layout == "strided" else o.T)).to(dev)       # [n, 3] | [3, n]
    w, i, pdf = target.evalp_is_proxy(proxy, d1, d2, do, tparams, params)
    torch.cuda.synchronize()
    w, i = w.cpu().numpy(), i.cpu().numpy()
    return (w, i, pdf.cpu().numpy()) if layout == "strided" else (w.T, i.T, pdf.cpu().numpy())


@pytest.mark.parametrize("target,proxy", cases.GPU_PAIRS, ids=lambda v: v)
def test_every_pair_equals_the_composed_oracle(objects, target, proxy):
    want, (o, u1, u2) = cases.expected(target, proxy, N)
    t, p, pp = objects("target", target), objects("proxy", proxy), cases.product_params(proxy)
    for layout in ("host", "dense", "strided"):
        cases.assert_same(f"{target} <- {proxy}, {layout}, n = {N}", _run(t, p, pp, u1, u2, o, layout), want, target, o)
    # every unit is independent: a prefix of the batch has the prefix of the results
    for n in DEVICE_SIZES:
        for layout in ("dense", "strided"):
            cases.assert_same(f"{target} <- {proxy}, {layout}, n = {n}", _run(t, p, pp, u1[:n], u2[:n], o[:n], layout), [a[:n] for a in want], target, o[:n])
    for n in HOST_SIZES:
        cases.assert_same(f"{target} <- {proxy}, host, n = {n}", _run(t, p, pp, u1[:n], u2[:n], o[:n], "host"), [a[:n] for a in want], target, o[:n])


def test_large_host_batches_take_the_chunked_pipeline(objects, monkeypatch):
    """host batches of two chunks or more are cut into chunks whose copies overlap the kernels, as for sample / evalp_is; the chunk
    size is lowered so that a small batch qualifies, and DJB_HOST_PIPE_REQUIRE turns "fell back to the plain path" into an error"""
    want, (o, u1, u2) = cases.expected("abc", "ggx_ell", N)
    monkeypatch.setenv("DJB_HOST_PIPE_CHUNK", "32768")
    monkeypatch.setenv("DJB_HOST_PIPE_REQUIRE", "1")
    got = _run(objects("target", "abc"), objects("proxy", "ggx_ell"), cases.product_params("ggx_ell"), u1, u2, o, "host")
    cases.assert_same("abc <- ggx, chunked host batch", got, want)


def _near_normal_block(n):
    """o within 1e-3 rad of the normal, a quarter of them exactly on it, and a bulk of ordinary directions behind"""
    from dj_brdf_amd import synth
    rng = np.random.default_rng(11)
    o = synth.directions_aos(n, synth.SEED_O).copy()
    m = n // 2
    t = rng.random(m) * 1e-3; ph = rng.random(m) * 6.2831853
    t[: m // 4] = 0
    o[:m] = np.stack([np.sin(t) * np.cos(ph), np.sin(t) * np.sin(ph), np.cos(t)], 1).astype(np.float32)
    return o, synth.uniforms(n, synth.SEED_U1), synth.uniforms(n, synth.SEED_U2)


def test_merl_pairs_that_tier_one_declines(gpu_ctx, objects, oracle):
    """A sharp GGX lobe seen from next to the normal puts h and d in and around the reference's 0.99999 snap zones, where the fp32 bin
    estimate declines and the exact index decides (the per-wave queue of djb_kernels_proxy.hip).  Bits equal to the composed oracle,
    with and without DJB_OPT_MERL_EXACT_ONLY."""
    n = 40_001
    o, u1, u2 = _near_normal_block(n)
    sharp = ("elliptic", 4.5e-3, 4.5e-3, 0.0)
    want = cases.compose(oracle, cases.oracle_target("merl"), cases.oracle_proxy("ggx_iso"), sharp, u1, u2, o)
    # a condition on the inputs: the oracle's pairs reach both the lanes tier 1 decides and the ones it declines
    live = want[1][:, 2] > 0
    import torch
    dev = f"cuda:{gpu_ctx.device}"
    stats = djb.merl_guard_stats(torch.from_numpy(np.ascontiguousarray(want[1][live].T)).to(dev), torch.from_numpy(np.ascontiguousarray(o[live].T)).to(dev), ctx=gpu_ctx)
    print("merl_guard_stats on the sampled pairs:", stats)
    assert stats["special"] + stats["ambiguous"] > 0 and stats["certain"] > 0, stats
    t, p, pp = objects("target", "merl"), objects("proxy", "ggx_iso"), djb.microfacet.params.isotropic(4.5e-3)
    for layout in ("dense", "strided", "host"):
        cases.assert_same(f"merl <- sharp ggx, {layout}", _run(t, p, pp, u1, u2, o, layout), want)
    djb.set_merl_exact_only(gpu_ctx, True)
    try:
        for layout in ("dense", "strided"):
            cases.assert_same(f"merl <- sharp ggx, exact only, {layout}", _run(t, p, pp, u1, u2, o, layout), want)
    finally:
        djb.set_merl_exact_only(gpu_ctx, False)


def _status(ctx, target, proxy, n, mem_device):
    """the raw C call on n units -> (status, message)"""
    import torch
    lib = _lib.load()
    if mem_device:
        dev = f"cuda:{ctx.device}"
        o = torch.zeros((3, n), dtype=torch.float32, device=dev); o[2] = 1
        u = torch.full((n,), 0.5, dtype=torch.float32, device=dev)
        w, i, pdf = torch.zeros_like(o), torch.zeros_like(o), torch.zeros_like(u)
        ptr = lambda a: C.c_void_p(a.data_ptr())
    else:
        o = np.tile(np.float32([[0, 0, 1]]), (n, 1)); u = np.full(n, 0.5, np.float32)
        w, i, pdf = np.zeros_like(o), np.zeros_like(o), np.zeros_like(u)
        ptr = lambda a: C.c_void_p(a.ctypes.data)
    vo, vw, vi = djb._Vec(o), djb._Vec(w), djb._Vec(i)
    st = lib.djb_evalp_is_proxy_batch(ctx._h, target._h, proxy._h, C.c_int64(n), ptr(u), ptr(u), C.byref(vo.view), None, None,
                                      C.byref(vw.view), C.byref(vi.view), ptr(pdf), C.c_int(_lib.MEM_DEVICE if mem_device else _lib.MEM_HOST))
    return st, lib.djb_last_error().decode(errors="replace")


def test_pairs_outside_the_set_are_not_implemented(gpu_ctx, objects, oracle):
    NOT_IMPLEMENTED = 5
    lam, ggx, abc = objects("target", "lambert"), objects("proxy", "ggx_iso"), objects("target", "abc")
    for t, p in ((lam, ggx), (abc, lam), (ggx, ggx)):
        for n, mem_device in ((97, False), (4096, False), (1, True), (4096, True)):
            st, msg = _status(gpu_ctx, t, p, n, mem_device)
            assert st == NOT_IMPLEMENTED and "target kind" in msg and "proxy kind" in msg, (st, msg)
    # at and below the host-twin size the host path answers, for every pair of kinds
    o, u1, u2 = cases.sampler_inputs(N)
    n = 96
    want = cases.compose(oracle, cases.oracle_target("lambert"), cases.oracle_proxy("ggx_iso"), cases.PROXIES["ggx_iso"][1], u1[:n], u2[:n], o[:n])
    cases.assert_same("lambert <- ggx, host twin", _run(lam, ggx, cases.product_params("ggx_iso"), u1[:n], u2[:n], o[:n], "host"), want)
    want = cases.compose(oracle, cases.oracle_target("abc"), cases.oracle_proxy("lambert"), None, u1[:n], u2[:n], o[:n])
    cases.assert_same("abc <- lambert, host twin", _run(abc, lam, None, u1[:n], u2[:n], o[:n], "host"), want)


def test_objects_of_two_contexts_are_refused(gpu_ctx, objects):
    other = djb.Context(gpu_ctx.device)
    ggx_other = djb.ggx(ctx=other)
    for n, mem_device in ((4, False), (4096, False), (4096, True)):
        st, msg = _status(gpu_ctx, objects("target", "abc"), ggx_other, n, mem_device)
        assert st == 1 and "different contexts" in msg, (st, msg)


def test_fused_call_replays_from_a_captured_graph(gpu_ctx, objects):
    """after one warm-up call a device-memory call is one asynchronous launch: it can be captured and replayed (tests/test_gpu_graph_capture.py)"""
    import torch
    from dj_brdf_amd import synth
    lib = _lib.load()
    n = 1 << 16
    dev = f"cuda:{gpu_ctx.device}"
    o = djb.gen_directions(n, synth.SEED_O, ctx=gpu_ctx); o[2].abs_()
    u1 = djb.gen_uniforms(n, synth.SEED_U1, ctx=gpu_ctx); u2 = djb.gen_uniforms(n, synth.SEED_U2, ctx=gpu_ctx)
    vo = djb._Vec(o)
    calls, keep = [], []
    for target, proxy in (("merl", "ggx_iso"), ("abc", "tabular"), ("utia", "tabular_aniso"), ("sgd", "beckmann_ell")):
        t, p, pp = objects("target", target), objects("proxy", proxy), cases.product_params(proxy)
        w, i = torch.zeros((3, n), dtype=torch.float32, device=dev), torch.zeros((3, n), dtype=torch.float32, device=dev)
        pdf = torch.zeros(n, dtype=torch.float32, device=dev)
        vw, vi = djb._Vec(w), djb._Vec(i)
        keep.extend([t, p, pp, vw, vi])

        def launch(t=t, p=p, pp=pp, vw=vw, vi=vi, pdf=pdf):
            _lib.check(lib.djb_evalp_is_proxy_batch(gpu_ctx._h, t._h, p._h, C.c_int64(n), C.c_void_p(u1.data_ptr()), C.c_void_p(u2.data_ptr()),
                                                    C.byref(vo.view), None, djb._params_ptr(pp), C.byref(vw.view), C.byref(vi.view),
                                                    C.c_void_p(pdf.data_ptr()), C.c_int(_lib.MEM_DEVICE)))
        calls.append((f"{target} <- {proxy}", launch, (w, i, pdf)))
    want, = graph_replay(gpu_ctx, lambda: [launch() for _, launch, _ in calls], [a for _, _, outs in calls for a in outs], [lambda: None])
    for k, (name, _, _) in enumerate(calls):          # one data set, resident; outputs 3 k .. 3 k + 2 are this pair's weight, i, pdf
        assert want[3 * k + 2].abs().sum() > 0, name


def test_contract_option_changes_no_bit(gpu_ctx, objects):
    want = {}
    pairs = (("abc", "ggx_ell"), ("sgd", "beckmann_iso"), ("utia", "ggx_iso"), ("merl", "tabular"))
    for target, proxy in pairs:
        want[target, proxy] = cases.expected(target, proxy, N)
    djb.set_contract_1e5(gpu_ctx, True)
    try:
        for target, proxy in pairs:
            res, (o, u1, u2) = want[target, proxy]
            got = _run(objects("target", target), objects("proxy", proxy), cases.product_params(proxy), u1, u2, o, "dense")
            cases.assert_same(f"{target} <- {proxy} under DJB_OPT_CONTRACT_1E5", got, res, target, o)
    finally:
        djb.set_contract_1e5(gpu_ctx, False)
