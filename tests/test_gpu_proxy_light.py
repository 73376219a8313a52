"""The light-sample call on the GPU (k_evalp_pdf_proxy, djb_kernels_proxy_light.hip: one launch per batch): evalp of the target and the
proxy's pdf for given pairs, every pair of kinds against the oracle's separate operators guarded as the plugins guard them
(tests/proxy_light_cases.py) -- bits equal in host, dense and strided layouts, at the sizes where a tile bound, the queue's flush trip or
the host-twin boundary can go wrong -- the MERL fall-back, the pairs the kernels do not serve, objects of two contexts, the chunked
host pipeline, graph capture, and the contract option."""
import ctypes as C

import numpy as np
import pytest

import proxy_light_cases as cases
from dj_brdf_amd import _lib, djb
from hit_calls import graph_replay

pytestmark = pytest.mark.gpu
N = cases.N
# around a wave and around each of the three workgroup sizes (256; 512 and 1024 with a tabular_anisotropic proxy)
DEVICE_SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
HOST_SIZES = (96, 97)                                 # the host twin answers up to DJB_SCALAR_HOST_MAX = 96 units
NOT_IMPLEMENTED = 5


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


def _run(target, proxy, params, i, o, layout, tparams=None):
    """one call in the given layout -> (fr [n,3], pdf [n]) as numpy"""
    import torch
    if layout == "host":
        return target.evalp_pdf_proxy(proxy, i, o, tparams, params)
    dev = f"cuda:{target.ctx.device}"
    di, do = (torch.from_numpy(np.ascontiguousarray(a if layout == "strided" else a.T)).to(dev) for a in (i, o))     # [n, 3] | [3, n]
    fr, pdf = target.evalp_pdf_proxy(proxy, di, do, tparams, params)
    torch.cuda.synchronize()
    fr = fr.cpu().numpy()
    return (fr if layout == "strided" else fr.T), pdf.cpu().numpy()


@pytest.mark.parametrize("target,proxy", cases.GPU_PAIRS, ids=lambda v: v)
def test_every_pair_equals_the_oracle(objects, target, proxy):
    i, o = cases.inputs()
    want = cases.expected(target, proxy)
    t, p, pp = objects("target", target), objects("proxy", proxy), cases.product_params(proxy)
    for layout in ("host", "dense", "strided"):
        cases.assert_same(f"{target} <- {proxy}, {layout}, n = {N}", _run(t, p, pp, i, o, layout), want, target, i, o)


@pytest.mark.parametrize("target,proxy", cases.GPU_PAIRS, ids=lambda v: v)
def test_prefix_sizes(objects, target, proxy):
    """every unit is independent: a prefix of the batch has the prefix of the results.  The prefixes start inside the specular block
    (non-zero pdfs for every lobe) and, for the host sizes, at the start of the batch"""
    i, o = cases.inputs()
    want = cases.expected(target, proxy)
    t, p, pp = objects("target", target), objects("proxy", proxy), cases.product_params(proxy)
    s0 = cases.light.SPECULAR[0] - 300                   # 300 ordinary pairs, then the specular block
    for n in DEVICE_SIZES:
        a, b = i[s0:s0 + n], o[s0:s0 + n]
        for layout in ("dense", "strided"):
            cases.assert_same(f"{target} <- {proxy}, {layout}, n = {n}", _run(t, p, pp, a, b, layout), [w[s0:s0 + n] for w in want], target, a, b)
    for n in HOST_SIZES:
        for k0 in (0, s0):
            a, b = i[k0:k0 + n], o[k0:k0 + n]
            cases.assert_same(f"{target} <- {proxy}, host, n = {n}", _run(t, p, pp, a, b, "host"), [w[k0:k0 + n] for w in want], target, a, b)


def test_large_host_batches_take_the_chunked_pipeline(objects, monkeypatch):
    """host batches of two chunks or more are cut into chunks whose copies overlap the kernels; the chunk size is lowered so that a
    small batch qualifies, and DJB_HOST_PIPE_REQUIRE turns "fell back to the plain path" into an error"""
    i, o = cases.inputs()
    reps = 3                                             # 120 003 pairs: three full chunks and a ragged one
    bi, bo = np.tile(i, (reps, 1)), np.tile(o, (reps, 1))
    want = [np.concatenate([w] * reps) for w in cases.expected("abc", "ggx_ell")]
    monkeypatch.setenv("DJB_HOST_PIPE_CHUNK", "32768")
    monkeypatch.setenv("DJB_HOST_PIPE_REQUIRE", "1")
    got = _run(objects("target", "abc"), objects("proxy", "ggx_ell"), cases.product_params("ggx_ell"), bi, bo, "host")
    cases.assert_same("abc <- ggx, chunked host batch", got, want)


def test_merl_pairs_that_tier_one_declines(gpu_ctx, objects, oracle):
    """o next to the normal and i next to its mirror direction put h and d in and around the reference's snap zones, where the fp32
    bin estimate declines and the exact index decides (the per-wave queue of djb_kernels_proxy_light.hip).  Bits equal to the oracle,
    with and without DJB_OPT_MERL_EXACT_ONLY."""
    import torch
    _, i, o = cases.declined_block()
    dev = f"cuda:{gpu_ctx.device}"
    stats = djb.merl_guard_stats(torch.from_numpy(np.ascontiguousarray(i.T)).to(dev), torch.from_numpy(np.ascontiguousarray(o.T)).to(dev), ctx=gpu_ctx)
    print("merl_guard_stats on the near-normal block:", stats)
    assert stats["ambiguous"] + stats["special"] >= 64 and stats["certain"] > 0 and stats["mismatch"] == 0, stats
    sharp = ("elliptic", 4.5e-3, 4.5e-3, 0.0)
    want = cases.expected_on(oracle, "merl", "ggx_iso", i, o, sharp)
    assert (want[1] > 0).sum() > len(i) // 4 and np.abs(want[0]).sum() > 0
    t, p, pp = objects("target", "merl"), objects("proxy", "ggx_iso"), djb.microfacet.params.isotropic(4.5e-3)
    got = {}
    for exact in (False, True):
        djb.set_merl_exact_only(gpu_ctx, exact)
        try:
            for layout in ("dense", "strided"):
                got[exact, layout] = _run(t, p, pp, i, o, layout)
                cases.assert_same(f"merl <- sharp ggx, {layout}, exact only = {exact}", got[exact, layout], want)
        finally:
            djb.set_merl_exact_only(gpu_ctx, False)
    for layout in ("dense", "strided"):
        cases.assert_same(f"{layout}: exact only against two tiers", got[True, layout], got[False, layout])


def _status(ctx, target, proxy, n, mem_device):
    """the raw C call on n units -> (status, message)"""
    import torch
    lib = _lib.load()
    if mem_device:
        dev = f"cuda:{ctx.device}"
        d = torch.zeros((3, n), dtype=torch.float32, device=dev); d[2] = 1
        fr, pdf = torch.zeros_like(d), torch.zeros(n, dtype=torch.float32, device=dev)
        ptr = lambda a: C.c_void_p(a.data_ptr())
    else:
        d = np.tile(np.float32([[0, 0, 1]]), (n, 1))
        fr, pdf = np.zeros_like(d), np.zeros(n, np.float32)
        ptr = lambda a: C.c_void_p(a.ctypes.data)
    vd, vfr = djb._Vec(d), djb._Vec(fr)
    st = lib.djb_evalp_pdf_proxy_batch(ctx._h, target._h, proxy._h, C.c_int64(n), C.byref(vd.view), C.byref(vd.view), None, None,
                                       C.byref(vfr.view), ptr(pdf), C.c_int(_lib.MEM_DEVICE if mem_device else _lib.MEM_HOST))
    return st, lib.djb_last_error().decode(errors="replace")


def test_pairs_outside_the_set_are_not_implemented(gpu_ctx, objects, oracle):
    lam, ggx, abc = objects("target", "lambert"), objects("proxy", "ggx_iso"), objects("target", "abc")
    for t, p in ((lam, ggx), (abc, lam), (ggx, ggx)):
        for n, mem_device in ((97, False), (4096, False), (1, True), (4096, True)):
            st, msg = _status(gpu_ctx, t, p, n, mem_device)
            assert st == NOT_IMPLEMENTED and "target kind" in msg and "proxy kind" in msg, (st, msg)
    # at and below the host-twin size the host path answers, for every pair of kinds
    n, s0 = 96, cases.light.SPECULAR[0] - 48
    i, o = (a[s0:s0 + n] for a in cases.inputs())
    want = cases.expected_on(oracle, "lambert", "ggx_iso", i, o)
    cases.assert_same("lambert <- ggx, host twin", _run(lam, ggx, cases.product_params("ggx_iso"), i, o, "host"), want)
    want = cases.expected_on(oracle, "abc", "lambert", i, o)
    cases.assert_same("abc <- lambert, host twin", _run(abc, lam, None, i, o, "host"), want)
    assert (want[1] > 0).any() and np.abs(want[0]).sum() > 0


def test_objects_of_two_contexts_are_refused(gpu_ctx, objects):
    other = djb.Context(gpu_ctx.device)
    ggx_other = djb.ggx(ctx=other)
    for n, mem_device in ((4, False), (4096, False), (4096, True)):
        st, msg = _status(gpu_ctx, objects("target", "abc"), ggx_other, n, mem_device)
        assert st == 1 and "different contexts" in msg, (st, msg)


def test_fused_call_replays_from_a_captured_graph(gpu_ctx, objects):
    """after one warm-up call a device-memory call is one asynchronous launch: it can be captured and replayed"""
    import torch
    from dj_brdf_amd import synth
    lib = _lib.load()
    n = 1 << 16
    dev = f"cuda:{gpu_ctx.device}"
    o = djb.gen_directions(n, synth.SEED_O, ctx=gpu_ctx); o[2].abs_()
    i = djb.gen_directions(n, synth.SEED_I, ctx=gpu_ctx); i[2, : n - n // 8].abs_()          # the last eighth keeps its guarded pairs
    vi, vo = djb._Vec(i), djb._Vec(o)
    calls, keep = [], []
    for target, proxy in (("merl", "ggx_iso"), ("abc", "tabular"), ("utia", "tabular_aniso"), ("sgd", "beckmann_ell")):
        t, p, pp = objects("target", target), objects("proxy", proxy), cases.product_params(proxy)
        fr, pdf = torch.zeros((3, n), dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
        vfr = djb._Vec(fr)
        keep.extend([t, p, pp, vfr])

        def launch(t=t, p=p, pp=pp, vfr=vfr, pdf=pdf):
            _lib.check(lib.djb_evalp_pdf_proxy_batch(gpu_ctx._h, t._h, p._h, C.c_int64(n), C.byref(vi.view), C.byref(vo.view), None,
                                                     djb._params_ptr(pp), C.byref(vfr.view), C.c_void_p(pdf.data_ptr()), C.c_int(_lib.MEM_DEVICE)))
        calls.append((f"{target} <- {proxy}", launch, (fr, pdf)))
    want, = graph_replay(gpu_ctx, lambda: [launch() for _, launch, _ in calls], [a for _, _, outs in calls for a in outs], [lambda: None])
    for k, (name, _, _) in enumerate(calls):          # one data set, resident; outputs 2 k and 2 k + 1 are this pair's fr and pdf
        assert want[2 * k + 1].abs().sum() > 0 and want[2 * k].abs().sum() > 0, name


def test_contract_option_changes_no_bit(gpu_ctx, objects):
    i, o = cases.inputs()
    pairs = (("abc", "ggx_ell"), ("sgd", "beckmann_iso"), ("utia", "ggx_iso"), ("merl", "tabular"))
    want = {pair: cases.expected(*pair) for pair in pairs}
    djb.set_contract_1e5(gpu_ctx, True)
    try:
        for target, proxy in pairs:
            got = _run(objects("target", target), objects("proxy", proxy), cases.product_params(proxy), i, o, "dense")
            cases.assert_same(f"{target} <- {proxy} under DJB_OPT_CONTRACT_1E5", got, want[target, proxy], target, i, o)
    finally:
        djb.set_contract_1e5(gpu_ctx, False)
