"""The light-sample call of MERL material sets on the GPU (k_merl_set_evalp_pdf, djb_kernels_merl_set.hip: one launch per batch): evalp of
the hit's material and the proxy's pdf with the hit's material's parameters for given pairs, against the oracle's per-material values
guarded as dj_merl guards them and selected by id (tests/merl_set_light_cases.py) -- bits equal in the three device layouts and at the
sizes where a tile bound can go wrong --, the exact-index fall-back, output bounds, all-guarded and all-inactive batches, graph capture,
and objects of other contexts.

Every device call of this file places its outputs between sentinel bands (one allocation: band, fr, band, pdf, band) and checks them."""
import ctypes as C

import numpy as np
import pytest

import merl_set_light_cases as cases
from dj_brdf_amd import _lib, djb

pytestmark = pytest.mark.gpu
KINDS = ("ggx", "beckmann")
LAYOUTS = ("soa", "soa16", "aos")            # dense from a 4-byte-aligned start, dense from 16-byte-aligned starts, strided records
RAGGED = (1, 63, 64, 65, 255, 256, 257, 4097)
SENT_BITS = 0x7FC0DEAD


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


def _dev(ctx):
    return f"cuda:{ctx.device}"


class Banded:
    """float planes of n elements in ONE sentinel-filled device allocation, a band before, between and after them.
    layout soa: 67-element bands (a plane starts 4-byte-aligned only); soa16: every plane starts 16-byte-aligned; aos: the first three
    planes are the components of n records of 3 (stride 3), further planes are plain arrays behind them"""

    def __init__(self, torch, dev, n, planes, layout):
        self.torch, self.n, self.aos = torch, n, layout == "aos"
        pad = 64 if layout == "soa16" else 67
        body = -(-n // 4) * 4 if layout == "soa16" else n
        self.start, at = [], pad
        if self.aos:
            self.start += [at, at + 1, at + 2]
            at += 3 * n + pad
            planes -= 3
        for _ in range(planes):
            self.start.append(at)
            at += body + pad
        self.t = torch.empty(at, dtype=torch.float32, device=dev)
        self.t.view(torch.int32).fill_(SENT_BITS)

    def _slice(self, k):
        step = 3 if self.aos and k < 3 else 1
        return slice(self.start[k], self.start[k] + step * (self.n - 1) + 1, step)

    def plane(self, k):
        return self.t[self._slice(k)]

    def ptr(self, k):
        return self.t.data_ptr() + 4 * self.start[k]

    def view(self):
        v = _lib.Vec3View()
        v.x, v.y, v.z, v.stride = self.ptr(0), self.ptr(1), self.ptr(2), 3 if self.aos else 1
        return v

    def fill(self, k, a):
        self.plane(k).copy_(self.torch.from_numpy(np.ascontiguousarray(a)).to(self.t.device))

    def get(self, k):
        return self.plane(k).cpu().numpy()

    def check(self, what, written=True):
        bits = self.t.view(self.torch.int32)
        inside = self.torch.zeros_like(bits, dtype=self.torch.bool)
        for k in range(len(self.start)):
            inside[self._slice(k)] = True
        sent = bits == SENT_BITS
        assert bool(sent[~inside].all()), f"{what}: a sentinel band was written ({int((~sent[~inside]).sum())} elements)"
        if written:
            assert not bool(sent[inside].any()), f"{what}: {int(sent[inside].sum())} output elements were never written"
        else:
            assert bool(sent[inside].all()), f"{what}: an output was written"


def _light(ctx, s, proxy, ids, i, o, layout, tag="", expect=0):
    """the C call on device memory in `layout`, outputs banded; returns (fr [n, 3], pdf [n]) -- or the status when it is not `expect`ed OK"""
    import torch
    dev, n = _dev(ctx), len(ids)
    out = Banded(torch, dev, n, 4, layout)
    if layout == "aos":                                  # strided inputs as well: [n, 3] records
        keep = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (i, o)]
        vin = [djb._Vec(t).view for t in keep]
    else:
        keep = Banded(torch, dev, n, 6, layout)
        vin = []
        for first, a in ((0, i), (3, o)):
            for c in range(3):
                keep.fill(first + c, a[:, c])
            v = _lib.Vec3View()
            v.x, v.y, v.z, v.stride = keep.ptr(first), keep.ptr(first + 1), keep.ptr(first + 2), 1
            vin.append(v)
    dids = torch.from_numpy(np.ascontiguousarray(ids)).to(dev)
    vout = out.view()
    st = _lib.load().djb_merl_set_evalp_pdf_proxy_batch(ctx._h, s._h, proxy._h, C.c_int64(n), C.c_void_p(dids.data_ptr()), C.byref(vin[0]),
                                                        C.byref(vin[1]), C.byref(vout), C.c_void_p(out.ptr(3)), C.c_int(_lib.MEM_DEVICE))
    torch.cuda.synchronize()
    if expect != 0:
        out.check(tag, written=False)
        return st, _lib.load().djb_last_error().decode(errors="replace")
    _lib.check(st)
    out.check(f"{tag} {layout} n={n}")
    return np.stack([out.get(c) for c in range(3)], 1), out.get(3)


# ------------------------------------------------------------------ 1. bits equal to the oracle selection
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("proxy", KINDS)
def test_equals_the_oracle_selection(gpu_ctx, mset, proxies, proxy, layout):
    ids, _ = cases.material_ids()
    i, o = cases.inputs()
    cases.assert_same(f"set <- {proxy}, {layout}", _light(gpu_ctx, mset, proxies[proxy], ids, i, o, layout, proxy), cases.expected(proxy))


def test_host_batches_are_staged_through_the_device(mset, proxies):
    ids, _ = cases.material_ids()
    i, o = cases.inputs()
    for proxy in KINDS:
        cases.assert_same(f"set <- {proxy}, host memory", mset.evalp_pdf_proxy(proxies[proxy], ids, i, o), cases.expected(proxy))


@pytest.mark.parametrize("proxy", KINDS)
def test_ragged_sizes(gpu_ctx, mset, proxies, proxy):
    """one wave, one block, and the block boundaries +- 1: units are independent, a prefix has the prefix's results"""
    ids, _ = cases.material_ids()
    i, o = cases.inputs()
    want = cases.expected(proxy)
    s0 = cases.SPECULAR[0]                               # the prefixes start inside the specular block: non-zero pdfs for every lobe
    for n in RAGGED:
        for layout in ("soa", "aos"):
            got = _light(gpu_ctx, mset, proxies[proxy], ids[s0:s0 + n], i[s0:s0 + n], o[s0:s0 + n], layout, proxy)
            cases.assert_same(f"set <- {proxy}, {layout}, n = {n}", got, [a[s0:s0 + n] for a in want])
    # ... and from the start of the batch, where the id changes every hit
    for n in RAGGED:
        cases.assert_same(f"set <- {proxy}, soa16, n = {n}", _light(gpu_ctx, mset, proxies[proxy], ids[:n], i[:n], o[:n], "soa16", proxy), [a[:n] for a in want])


# ------------------------------------------------------------------ 2. pairs tier 1 declines
def test_pairs_that_tier_one_declines(gpu_ctx, mset, proxies):
    import torch
    ids, i, o = cases.declined_block()
    dev = _dev(gpu_ctx)
    stats = djb.merl_guard_stats(torch.from_numpy(np.ascontiguousarray(i.T)).to(dev), torch.from_numpy(np.ascontiguousarray(o.T)).to(dev), ctx=gpu_ctx)
    print("merl_guard_stats on the near-normal block:", stats)
    assert stats["ambiguous"] + stats["special"] >= 64 and stats["certain"] > 0 and stats["mismatch"] == 0, stats
    for proxy in KINDS:
        want = cases.expected_on(proxy, ids, i, o)
        assert (want[1] > 0).sum() > len(ids) // 4 and np.abs(want[0]).sum() > 0
        got = {}
        for exact in (False, True):
            djb.set_merl_exact_only(gpu_ctx, exact)
            try:
                for layout in ("soa", "aos"):
                    got[exact, layout] = _light(gpu_ctx, mset, proxies[proxy], ids, i, o, layout, f"{proxy} exact only = {exact}")
                    cases.assert_same(f"{proxy}, {layout}, exact only = {exact}", got[exact, layout], want)
            finally:
                djb.set_merl_exact_only(gpu_ctx, False)
        for layout in ("soa", "aos"):
            cases.assert_same(f"{proxy}, {layout}: exact only against two tiers", got[True, layout], got[False, layout])


# ------------------------------------------------------------------ 3. bands
@pytest.mark.parametrize("layout", LAYOUTS)
def test_outputs_stay_inside_their_bands(gpu_ctx, mset, proxies, layout):
    """n = 4 099: margins before fr, between its planes, between fr and pdf and behind pdf are untouched, every output written"""
    ids, _ = cases.material_ids()
    i, o = cases.inputs()
    n, s0 = 4099, 1000                                   # [1000, 5099): the below-horizon, NaN and zero-vector blocks are inside
    for proxy in KINDS:
        want = cases.expected(proxy)
        got = _light(gpu_ctx, mset, proxies[proxy], ids[s0:s0 + n], i[s0:s0 + n], o[s0:s0 + n], layout, f"bands {proxy}")   # checks the bands
        cases.assert_same(f"bands {proxy} {layout}", got, [a[s0:s0 + n] for a in want])


# ------------------------------------------------------------------ 4. batches with nothing to evaluate
def test_all_inactive_and_all_guarded_batches(gpu_ctx, proxies):
    """every output bit is +0 (the sign included); the set is a valid one built from members"""
    n = 4099
    rng = np.random.default_rng(17)
    i, o = (a[:n].copy() for a in cases.inputs())
    members = cases.product_members(gpu_ctx)
    s = djb.merl_set(members, cases.product_params(), ctx=gpu_ctx)
    try:
        dead = rng.choice(cases.base.inactive_values(), n).astype(np.int32)
        live = (np.arange(n) % cases.M).astype(np.int32)
        below_i, below_o = i.copy(), o.copy()
        below_i[:, 2] = -np.abs(np.nan_to_num(i[:, 2], nan=0.5)); below_i[::7, 2] = 0.0; below_i[::11, 2] = -0.0
        below_o[:, 2] = -np.abs(np.nan_to_num(o[:, 2], nan=0.5)); below_o[::5, 2] = 0.0
        for proxy in KINDS:
            for layout in LAYOUTS:
                for tag, ids_, i_, o_ in (("inactive", dead, i, o), ("i below", live, below_i, o), ("o below", live, i, below_o),
                                          ("both below", live, below_i, below_o)):
                    fr, pdf = _light(gpu_ctx, s, proxies[proxy], ids_, i_, o_, layout, f"{tag} {proxy}")
                    assert not fr.view(np.uint32).any() and not pdf.view(np.uint32).any(), (tag, proxy, layout)
        # the same set answers an ordinary batch: it is a valid one
        ids, _ = cases.material_ids()
        s0 = cases.SPECULAR[0]
        fr, pdf = _light(gpu_ctx, s, proxies["ggx"], ids[s0:s0 + n], cases.inputs()[0][s0:s0 + n], cases.inputs()[1][s0:s0 + n], "soa")
        cases.assert_same("valid set", (fr, pdf), [a[s0:s0 + n] for a in cases.expected("ggx")])
    finally:
        s.close()
        for b in members:
            b.close()


# ------------------------------------------------------------------ 5. graph capture
def _hip_runtime():
    """the HIP runtime this process has loaded"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    return C.CDLL(paths.pop())


def test_replays_from_a_captured_graph(gpu_ctx, mset, proxies):
    import torch
    lib = _lib.load()
    n = 1 << 13
    dev = _dev(gpu_ctx)
    all_ids, _ = cases.material_ids()
    ai, ao = cases.inputs()
    s0 = cases.SPECULAR[0]
    sets = [(all_ids[k:k + n], ai[k:k + n], ao[k:k + n]) for k in (s0 - 2000, 1000, 20_000)]     # eager, replay 1, replay 2
    side = torch.cuda.Stream(device=gpu_ctx.device)
    with torch.cuda.stream(side):                        # the context follows torch's current stream
        ids = torch.zeros(n, dtype=torch.int32, device=dev)
        i, o, fr = (torch.zeros((3, n), dtype=torch.float32, device=dev) for _ in range(3))
        pdf = torch.zeros(n, dtype=torch.float32, device=dev)
        vi, vo, vfr = djb._Vec(i), djb._Vec(o), djb._Vec(fr)

        def put(k):
            ids.copy_(torch.from_numpy(np.ascontiguousarray(sets[k][0])).to(dev))
            i.copy_(torch.from_numpy(np.ascontiguousarray(sets[k][1].T)).to(dev)); o.copy_(torch.from_numpy(np.ascontiguousarray(sets[k][2].T)).to(dev))

        def launch():
            _lib.check(lib.djb_merl_set_evalp_pdf_proxy_batch(gpu_ctx._h, mset._h, proxies["beckmann"]._h, C.c_int64(n), C.c_void_p(ids.data_ptr()),
                                                              C.byref(vi.view), C.byref(vo.view), C.byref(vfr.view), C.c_void_p(pdf.data_ptr()),
                                                              C.c_int(_lib.MEM_DEVICE)))
        want = []
        for k in range(3):                               # eager: the results to hold the replays against
            put(k); launch(); side.synchronize()
            want.append((fr.clone(), pdf.clone()))
        assert not torch.equal(want[1][1].view(torch.int32), want[2][1].view(torch.int32)) and want[0][1].abs().sum() > 0
        fr.zero_(); pdf.zero_()
        side.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=side):
        launch()
    assert not fr.any() and not pdf.any(), "the call ran during capture instead of being recorded"
    # what was recorded: one kernel node, hence no edges and no parallel branches
    hip = _hip_runtime()
    graph = C.c_void_p(g.raw_cuda_graph())
    n_nodes, n_edges = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and hip.hipGraphGetEdges(graph, None, None, C.byref(n_edges)) == 0
    assert (n_nodes.value, n_edges.value) == (1, 0), (n_nodes.value, n_edges.value)
    node, kind = (C.c_void_p * 1)(), C.c_int(-1)
    assert hip.hipGraphGetNodes(graph, node, C.byref(n_nodes)) == 0 and hip.hipGraphNodeGetType(C.c_void_p(node[0]), C.byref(kind)) == 0
    assert kind.value == 0, f"node type {kind.value}, not a kernel node"
    for k in (1, 2):                                     # replayed twice, on changed inputs
        with torch.cuda.stream(side):
            put(k); fr.zero_(); pdf.zero_()
            side.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for a, e, name in zip((fr, pdf), want[k], ("fr", "pdf")):
            assert torch.equal(a.view(torch.int32), e.view(torch.int32)), f"replay {k}: {name} differs from the direct call"


# ------------------------------------------------------------------ 6. contexts
def test_objects_of_other_contexts_are_refused(gpu_ctx, mset, proxies):
    n = 257
    ids, _ = cases.material_ids()
    i, o = cases.inputs()
    s0 = cases.SPECULAR[0]
    a = (ids[s0:s0 + n], i[s0:s0 + n], o[s0:s0 + n])
    other = djb.Context(gpu_ctx.device)
    cpu = djb.cpu_context()
    cpu_set = djb.merl_set(cases.product_members(cpu)[:1], [djb.microfacet.params.isotropic(0.3)], ctx=cpu)
    try:
        for layout in ("soa", "aos"):
            st, msg = _light(gpu_ctx, mset, djb.ggx(ctx=other), *a, layout, "foreign proxy", expect=1)
            assert st == 1 and "different contexts" in msg, (st, msg)
            st, msg = _light(other, mset, djb.ggx(ctx=other), *a, layout, "foreign set", expect=1)
            assert st == 1 and "another context" in msg, (st, msg)
            st, msg = _light(gpu_ctx, cpu_set, proxies["ggx"], *a, layout, "cpu set", expect=1)
            assert st == 1 and "different back ends" in msg, (st, msg)
            st, msg = _light(gpu_ctx, mset, djb.ggx(ctx=cpu), *a, layout, "cpu proxy", expect=1)
            assert st == 1, (st, msg)
            st, msg = _light(gpu_ctx, mset, djb.tabular(djb.ggx(ctx=gpu_ctx), 16, True, ctx=gpu_ctx), *a, layout, "tabular proxy", expect=5)
            assert st == 5 and "ggx or beckmann" in msg, (st, msg)
        cases.assert_same("own objects", _light(gpu_ctx, mset, proxies["ggx"], *a, "soa"), [w[s0:s0 + n] for w in cases.expected("ggx")])
    finally:
        cpu_set.close()
