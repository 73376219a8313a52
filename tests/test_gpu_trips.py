"""What a workgroup of the core kernels does after its first tile: every grid-stride kernel of csrc/djb_kernels_eval.hip and csrc/djb_kernels_sample.hip
(and k_utia_v2, the contract fix-up's rescan, the harness kernels) on a batch one ragged trip longer than its grid covers -- two for the two kernels
that carry a per-wave queue from trip to trip -- against the ORACLE's bits on every unit.

Cases, trip sizes and the blocks that make the per-wave queue counts known: tests/trip_cases.py (pinned on the CPU by tests/test_trip_cases_host.py).
Every call goes through the C ABI on device memory, dense [3, n] and strided [n, 3]; every output lies in an allocation prefilled with a sentinel, at
least one unit longer than the batch: a unit that was not written shows, and so does a write behind the end."""
import numpy as np
import pytest

import trip_cases as tc
from dj_brdf_amd import djb, synth
from param_space_cases import mk_params
from test_gpu_contract import check_contract, check_directions

pytestmark = pytest.mark.gpu
LAYOUTS = {"dense": "dense", "strided": "aos3"}


class Dev:
    """device copies of the tiled blocks and of the expected bits, kept for the module"""

    def __init__(self, ctx):
        import torch
        self.torch, self.ctx, self.dev = torch, ctx, tc.device_of(ctx)
        self._blocks, self._want = {}, {}

    def src(self, block, n):
        if block not in self._blocks:
            self._blocks[block] = dict(zip(("i", "o", "u1", "u2"), (tc.upload(self.torch, self.dev, a) for a in tc.BLOCKS[block]())))
        return {k: tc.tile_dev(t, n) for k, t in self._blocks[block].items()}

    def want_bits(self, spec, block, params, op, n):
        key = (spec, block, params, op)
        if key not in self._want:
            self._want[key] = tuple(tc.upload(self.torch, self.dev, tc.bits_i32(a)) for a in tc.expected(spec, block, params, op))
        return tuple(tc.tile_dev(t, n) for t in self._want[key])

    def run(self, b, spec, block, params, op, n, layout, tag, queued=None):
        """one call, every output against the tiled oracle's bits; the inputs unchanged"""
        tc.assert_second_trip_is_not_vacuous(tag, tc.expected(spec, block, params, op), queued)
        src = self.src(block, n)
        lay = {k: LAYOUTS[layout] for k in ("i", "o", "out", "w")}
        ins, outs = tc.call(self.ctx, b, op, n, src, mk_params(params) if params is not None else None, self.torch, self.dev, layouts=lay)
        for k, (out, want) in enumerate(zip(outs, self.want_bits(spec, block, params, op, n))):
            out.check_bits(f"{tag}, {op} output {k}, {layout}, n = {n}", want)
        tc.check_inputs_unchanged(f"{tag}, {op}, {layout}", ins, src)


@pytest.fixture(scope="module")
def D(gpu_ctx):
    import torch
    d = Dev(gpu_ctx)
    yield d
    d._blocks.clear(); d._want.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ k_eval_bk_sharp: the carried queue and the prefetched next tile
@pytest.mark.parametrize("trips", [2, 3])
@pytest.mark.parametrize("setup", tc.SHARP_SETUPS, ids=lambda s: f"{s[0][0]}-{'shadow' if s[1] else 'noshadow'}")
def test_sharp_lobe_beckmann(gpu_ctx, D, setup, trips):
    """eval, evalp, pdf, eval_pdf (cos 0 and 1) of the three sharp lobes: 4 096 * 256 pairs per trip (launch_eval_kind_fr: `blocks`).  Wave w of the sixteen
    workgroups that run every trip queues WAVE_COUNTS[w] pairs per trip: the residue of 1 <= c <= 31 is flushed after the loop (c >= 22: drained on the third
    trip), 32 <= c <= 63 drains entries of two trips together, c = 64 drains every trip, c = 0 never"""
    spec = ("mf", "beckmann") + setup
    b = tc.product_object(spec, gpu_ctx)
    queued = tc.sharp_block()[2]
    n = tc.units("sharp", trips)
    for p in tc.SHARP_LOBES:
        for op in tc.EVAL_OPS:
            for layout in LAYOUTS:
                D.run(b, spec, "sharp", p, op, n, layout, f"sharp lobe {setup} {p}, {trips} trips", queued)


# ------------------------------------------------------------------ k_sample_bk: the carried queue of deferred samples
@pytest.mark.parametrize("trips", [2, 3])
@pytest.mark.parametrize("spec", tc.SAMPLER_SPECS, ids=lambda s: s[2][0])
def test_beckmann_sampler(gpu_ctx, D, spec, trips):
    """sample and evalp_is: 5 120 * 256 samples per trip (grid_persistent); the deferred families of trip_cases.sampler_block fill the queues as above"""
    b = tc.product_object(spec, gpu_ctx)
    deferred = tc.sampler_block()[3]
    n = tc.units("sampler", trips)
    for p in tc.SAMPLER_PARAMS:
        for op in tc.SAMPLE_OPS:
            for layout in LAYOUTS:
                D.run(b, spec, "sampler", p, op, n, layout, f"beckmann sampler {spec[2][0]} {p}, {trips} trips", deferred)


@pytest.mark.parametrize("trips", [2, 3])
def test_beckmann_sample_rng_equals_the_array_path(gpu_ctx, D, trips):
    """sample_rng (the RNG instantiations of k_sample_bk) against the array path -- held against the oracle above -- fed with gen_uniforms at the same n and
    start: the same bits, unit for unit"""
    torch = D.torch
    spec = tc.SAMPLER_SPECS[0]
    b = tc.product_object(spec, gpu_ctx)
    n, start = tc.units("sampler", trips), 17
    src = D.src("sampler", n)
    src["u1"], src["u2"] = djb.gen_uniforms(n, synth.SEED_U1, start, ctx=gpu_ctx), djb.gen_uniforms(n, synth.SEED_U2, start, ctx=gpu_ctx)
    for p in tc.SAMPLER_PARAMS:
        up = mk_params(p) if p is not None else None
        for layout in LAYOUTS:
            lay = {k: LAYOUTS[layout] for k in ("o", "out")}
            _, (ref,) = tc.call(gpu_ctx, b, "sample", n, src, up, torch, D.dev, layouts=lay)
            _, (got,) = tc.call(gpu_ctx, b, "sample", n, src, up, torch, D.dev, layouts=lay, rng=(synth.SEED_U1, synth.SEED_U2, start))
            ref.check_frame(f"array path {p} {layout}")
            got.check_bits(f"sample_rng {p}, {layout}, n = {n}", ref.values_bits()[1])


@pytest.mark.parametrize("ndf", ["beckmann", "ggx"])
def test_contract_sampler(gpu_ctx, D, ndf):
    """DJB_OPT_CONTRACT_1E5: `sample` of Beckmann and GGX (the CT instantiations of k_sample_bk) within the contract of tests/test_gpu_contract.py --
    1e-5 per component, the reference's degenerate answers --; Beckmann's evalp_is keeps the reference's direction bits, weight and pdf within 1e-5 relative"""
    torch = D.torch
    n = tc.units("sampler")
    src = D.src("sampler", n)
    o_host = tc.tiled(tc.sampler_block()[2], n)
    djb.set_contract_1e5(gpu_ctx, True)
    try:
        for spec in tc.SAMPLER_SPECS if ndf == "beckmann" else (tc.GGX_CONTRACT_SAMPLER,):
            b = tc.product_object(spec, gpu_ctx)
            for p in tc.SAMPLER_PARAMS:
                up = mk_params(p) if p is not None else None
                for layout in LAYOUTS:
                    lay = {k: LAYOUTS[layout] for k in ("o", "out", "w")}
                    tag = f"contract {ndf} {spec[2][0]} {p} {layout}"
                    if spec[2] == tc.FRESNEL_IDEAL:
                        _, (got,) = tc.call(gpu_ctx, b, "sample", n, src, up, torch, D.dev, layouts=lay)
                        got.check_frame(tag + " sample")
                        worst = check_directions(tag + " sample", got.values(), tc.tiled(tc.oracle_output(spec, "sampler", p, "sample"), n), o_host)
                        print(f"{tag}: sample, worst component difference {worst:.3e}")
                    if ndf == "beckmann":
                        _, (w, si, pdf) = tc.call(gpu_ctx, b, "evalp_is", n, src, up, torch, D.dev, layouts=lay)
                        ww, wi, wpdf = D.want_bits(spec, "sampler", p, "evalp_is", n)
                        si.check_bits(tag + " evalp_is direction", wi)
                        w.check_frame(tag + " evalp_is weight"); pdf.check_frame(tag + " evalp_is pdf")
                        check_contract(tag + " evalp_is weight", w.values(), tc.tiled(tc.oracle_output(spec, "sampler", p, "is_w"), n))
                        check_contract(tag + " evalp_is pdf", pdf.values(), tc.tiled(tc.oracle_output(spec, "sampler", p, "is_pdf"), n))
    finally:
        djb.set_contract_1e5(gpu_ctx, False)


# ------------------------------------------------------------------ k_eval / k_sample of the kinds on the capped grid
@pytest.mark.parametrize("name", list(tc.CAPPED))
def test_capped_kinds(gpu_ctx, D, name):
    """eval / evalp / pdf / eval_pdf and sample / evalp_is of the table-driven and fitted kinds, MERL and UTIA on their exact-only forms (k_eval<MERL / UTIA>):
    4 096 * 256 units per trip, 2 048 * 1 024 for tabular_anisotropic's eval: the LDS tables staged once serve the second tile, the scalar bound of the ragged
    tile is derived again"""
    spec, block, plist, trip_eval, trip_sample = tc.CAPPED[name]
    b = tc.product_object(spec, gpu_ctx)
    knob = {"merl_exact": djb.set_merl_exact_only, "utia_exact": djb.set_utia_exact_only}.get(name)
    if knob:
        knob(gpu_ctx, True)
    try:
        for p in plist:
            for op in tc.EVAL_OPS + tc.SAMPLE_OPS:
                n = tc.units(trip_eval if op in tc.EVAL_OPS else trip_sample)
                for layout in LAYOUTS:
                    D.run(b, spec, block, p, op, n, layout, f"{name} {p}")
    finally:
        if knob:
            knob(gpu_ctx, False)


@pytest.mark.parametrize("cap", [-1, 0], ids=["default", "worklist0"])
def test_utia_two_tier_single_material(gpu_ctx, D, cap):
    """k_utia_v2 (16 384 * 256 pairs per trip) with its fix-up kernel, and with the worklist forced to overflow (the exact kernel redoes the batch)"""
    b = tc.product_object("utia_drawn", gpu_ctx)
    n = tc.units("utia_v2")
    djb.set_test_worklist_cap(gpu_ctx, cap)
    try:
        for op in ("eval", "evalp"):
            for layout in LAYOUTS:
                D.run(b, "utia_drawn", "finite", None, op, n, layout, f"utia two-tier, worklist cap {cap}")
    finally:
        djb.set_test_worklist_cap(gpu_ctx, -1)


@pytest.mark.parametrize("case", tc.FIXUP, ids=lambda c: c[0] if isinstance(c[0], str) else c[0][1])
def test_contract_fixup_rescan(gpu_ctx, D, case):
    """contract mode with the worklist cap forced to 0: the fix-up kernel rescans the whole batch (a grid-stride loop of its own) and the exact kernel
    answers the tail behind the last multiple of four: every value inside the contract of tests/test_gpu_contract.py"""
    spec, p = case
    b = tc.product_object(spec, gpu_ctx)
    n = tc.units("capped")
    assert n % 4 == 1
    src = D.src("hostile", n)
    want = tc.tiled(tc.oracle_output(spec, "hostile", p, "evalp"), n)
    djb.set_contract_1e5(gpu_ctx, True)
    djb.set_test_worklist_cap(gpu_ctx, 0)
    try:
        _, (out,) = tc.call(gpu_ctx, b, "evalp", n, src, mk_params(p) if p is not None else None, D.torch, D.dev)
        out.check_frame(f"contract fix-up {spec}")
        print(f"contract fix-up {spec}: max relative error", check_contract(f"contract fix-up {spec}", out.values(), want))
    finally:
        djb.set_test_worklist_cap(gpu_ctx, -1)
        djb.set_contract_1e5(gpu_ctx, False)


# ------------------------------------------------------------------ the harness kernels on the same cap
def test_harness_kernels(gpu_ctx, D, oracle):
    """gen_directions / gen_uniforms against synth, io_to_hd -> hd_to_io and merl_index against the oracle, one ragged trip beyond the 4 096 workgroups"""
    import ctypes as C
    from dj_brdf_amd import _lib
    torch, lib = D.torch, _lib.load()
    n, start = tc.units("capped"), 5
    mem = C.c_int(_lib.MEM_HOST if gpu_ctx.is_cpu else _lib.MEM_DEVICE)
    g = tc.Arr(torch, D.dev, n, 3); vg = g.view()
    _lib.check(lib.djb_gen_directions(gpu_ctx._h, C.c_int64(n), C.c_uint32(synth.SEED_I), C.c_uint64(start), C.byref(vg)))
    gu = tc.Arr(torch, D.dev, n, 1)
    _lib.check(lib.djb_gen_uniforms(gpu_ctx._h, C.c_int64(n), C.c_uint32(synth.SEED_U1), C.c_uint64(start), C.c_void_p(gu.ptr())))
    gpu_ctx.synchronize()
    g.check_bits("gen_directions", tc.upload(torch, D.dev, tc.bits_i32(synth.directions_aos(n, synth.SEED_I, start))))
    gu.check_bits("gen_uniforms", tc.upload(torch, D.dev, tc.bits_i32(synth.rng_uniforms(n, synth.SEED_U1, start))))
    i, o, _, _ = tc.hostile_block()
    wh, wd = oracle.io_to_hd(i, o)
    wi, wo = oracle.hd_to_io(wh, wd)
    src = D.src("hostile", n)
    for layout in LAYOUTS:
        mk = lambda data=None: tc.Arr(torch, D.dev, n, 3, LAYOUTS[layout], 0, data)
        ai, ao, ah, ad, bi, bo = mk(src["i"]), mk(src["o"]), mk(), mk(), mk(), mk()
        views = [a.view() for a in (ai, ao, ah, ad, bi, bo)]
        _lib.check(lib.djb_io_to_hd_batch(gpu_ctx._h, C.c_int64(n), C.byref(views[0]), C.byref(views[1]), C.byref(views[2]), C.byref(views[3]), mem))
        _lib.check(lib.djb_hd_to_io_batch(gpu_ctx._h, C.c_int64(n), C.byref(views[2]), C.byref(views[3]), C.byref(views[4]), C.byref(views[5]), mem))
        gpu_ctx.synchronize()
        for a, w, what in ((ah, wh, "io_to_hd h"), (ad, wd, "io_to_hd d"), (bi, wi, "hd_to_io i"), (bo, wo, "hd_to_io o")):
            a.check_bits(f"{what}, {layout}", tc.tile_dev(tc.upload(torch, D.dev, tc.bits_i32(w)), n))
    fi, fo, _, _ = tc.finite_block()
    want = tc.tile_dev(tc.upload(torch, D.dev, oracle.merl_index(fi, fo)), n)
    fsrc = D.src("finite", n)
    for layout in LAYOUTS:
        a, b = (fsrc["i"], fsrc["o"]) if layout == "strided" else (fsrc["i"].T.contiguous(), fsrc["o"].T.contiguous())
        got = djb.merl_index(a, b, ctx=gpu_ctx)
        assert torch.equal(got, want), f"merl_index, {layout}: {int((got != want).sum())} of {n} indices differ"
    assert len(np.unique(oracle.merl_index(fi, fo)[:tc.BLOCK_N - tc.RAGGED])) > 64
