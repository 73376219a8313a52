"""Resident LEAN maps on the MI355X: the builder kernels, the pyramid, the lookup kernel and the MODE 2 per-pair kernels (lookup
fused into eval / sample) against the real reference's fixtures, the numpy restatement of include/djb_hip.h, the composed
two-call path and the CPU context.  Equal bits throughout (leanmap_cases.same: NaNs in the same places)."""
import gc

import numpy as np
import pytest

import leanmap_cases as lc
from dj_brdf_amd import djb, synth

pytestmark = pytest.mark.gpu
f32 = np.float32
TWIN_MAX = 96            # DJB_SCALAR_HOST_MAX: host-array calls up to this size are answered by the host twin


def test_level0_is_the_reference_tools_output(gpu_ctx):
    lc.check_level0_against_reference(gpu_ctx)


def test_moments_import_and_bias(gpu_ctx):
    lc.check_moments_import_and_bias(gpu_ctx)


def test_pyramid_and_lookup_match_the_definition_host_arrays(gpu_ctx):
    lc.check_pyramid_and_lookup(gpu_ctx)


def test_pyramid_and_lookup_match_the_definition_device_arrays(gpu_ctx):
    lc.check_pyramid_and_lookup(gpu_ctx, device="cuda:0")


def test_small_lookups_are_answered_by_the_host_twin_with_the_same_bits(gpu_ctx):
    for name, m, l0 in lc.all_maps(gpu_ctx):
        uv, lod = lc.hostile_coords(4096, m.levels, 3)
        big = m.lookup(uv, lod)
        for n in (1, 37, TWIN_MAX):
            assert lc.same(m.lookup(uv[:n], lod[:n]), big[:n]), (name, n)


def test_fused_calls_equal_lookup_then_lean_host_arrays(gpu_ctx):
    lc.check_fused_equals_composed(gpu_ctx, sizes=(37, 20000))          # 37: the host twin answers; 20000: the kernels


def test_fused_calls_equal_lookup_then_lean_device_arrays(gpu_ctx):
    lc.check_fused_equals_composed(gpu_ctx, sizes=(37, 20000), device="cuda:0")


def test_gpu_equals_cpu_context(gpu_ctx):
    """item 4: map building (all levels), lookup and the fused calls"""
    cpu = djb.cpu_context()
    g = lc.fixture()
    for (name, mg, _), (_, mc, _) in zip(lc.all_maps(gpu_ctx), lc.all_maps(cpu)):
        assert mg.levels == mc.levels
        for l in range(mg.levels):
            assert lc.same(mg.level(l), mc.level(l)), (name, l)
        uv, lod = lc.hostile_coords(50000, mg.levels, 29)
        assert lc.same(mg.lookup(uv, lod), mc.lookup(uv, lod)), name
    for name in lc.MAPS:
        d = g[f"dmap_{name}"]
        a, b = djb.leanmap.from_dmap(d, 4.0, 0.02, ctx=gpu_ctx), djb.leanmap.from_dmap(d, 4.0, 0.02, ctx=cpu)
        for l in range(a.levels):
            assert lc.same(a.level(l), b.level(l)), (name, l)
    n = 20000
    mg, mc = (djb.leanmap.from_nmap(g["nmap_b128x128_s01"], 1e-5, ctx=c) for c in (gpu_ctx, cpu))
    i, o = synth.directions_aos(n, synth.SEED_I), synth.directions_aos(n, synth.SEED_O)
    u1, u2 = synth.uniforms(n, synth.SEED_U1), synth.uniforms(n, synth.SEED_U2)
    uv, lod = lc.hostile_coords(n, mg.levels, 31)
    base = lc.P.elliptic(0.12, 0.2, 0.3)
    for (lname, bg), (_, bc) in zip(lc.lobes(gpu_ctx), lc.lobes(cpu)):
        for filtering in (True, False):
            a = bg.eval_leanmap(i, o, mg, uv, lod, base, 0.8, want="evalp+pdf", return_params=True, filtering=filtering)
            c = bc.eval_leanmap(i, o, mc, uv, lod, base, 0.8, want="evalp+pdf", return_params=True, filtering=filtering)
            assert all(lc.same(x, y) for x, y in zip(a, c)), (lname, filtering)
            a = bg.sample_leanmap(u1, u2, o, mg, uv, lod, base, 0.8, return_params=True, filtering=filtering)
            c = bc.sample_leanmap(u1, u2, o, mc, uv, lod, base, 0.8, return_params=True, filtering=filtering)
            assert all(lc.same(x, y) for x, y in zip(a, c)), (lname, filtering, "sample")


def test_filtered_moments_widen_the_lobe(gpu_ctx):
    lc.check_lean_property(gpu_ctx)


def test_errors(gpu_ctx):
    lc.check_errors(gpu_ctx)


def test_a_map_belongs_to_its_context(gpu_ctx):
    """a CPU context's map on a GPU context and the reverse are invalid arguments, as for djb_brdf handles"""
    cpu = djb.cpu_context()
    nmap = lc.fixture()["nmap_n64x32_s01"]
    n = 1000
    i, uv = synth.directions_aos(n, 1), np.zeros((n, 2), f32)
    u = synth.uniforms(n, 2)
    for ctx, other in ((gpu_ctx, cpu), (cpu, gpu_ctx)):
        m, b = djb.leanmap.from_nmap(nmap, ctx=other), djb.beckmann(ctx=ctx)
        foreign = djb.leanmap(ctx); foreign._h = m._h            # the other context's handle presented to this context
        for call in (lambda: foreign.lookup(uv), lambda: foreign.lookup(uv[:8]),
                     lambda: b.eval_leanmap(i, i, m, uv, None, lc.P.isotropic(0.1), 1.0),
                     lambda: b.eval_leanmap(i[:8], i[:8], m, uv[:8], None, lc.P.isotropic(0.1), 1.0),
                     lambda: b.sample_leanmap(u, u, i, m, uv, None, lc.P.isotropic(0.1), 1.0)):
            with pytest.raises(djb.exc) as e:
                call()
            assert e.value.status == 1 and "different back ends" in str(e.value)
        foreign._h = None
        m.close()


def test_maps_give_their_hbm_back(gpu_ctx):
    import torch
    rng = np.random.default_rng(1)
    d = rng.integers(0, 256, (1024, 1024), dtype=np.uint8)
    uv = rng.random((4096, 2)).astype(f32)

    def one_round():
        m = djb.leanmap.from_dmap(d, 0.1, ctx=gpu_ctx)      # 1024 x 1024 x 32 B x 4/3 = 43 MiB
        m.lookup(uv); m.lookup(uv[:4])                        # the second builds the host copy for the twin
        m.close(); m.close()
    for _ in range(2): one_round()
    gc.collect(); torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(12): one_round()
    gc.collect(); torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 << 20, f"{(free0 - free1) / 2**20:.1f} MiB of HBM not returned after 12 maps"
    # a map may outlive the context that made it
    c = djb.Context(0)
    m = djb.leanmap.from_dmap(d[:64, :64], 0.1, ctx=c)
    c.close()
    m.close()


def test_map_records_through_the_per_hit_operators_against_the_oracle_device_arrays(gpu_ctx, oracle):
    """records every fixture map, the hostile map and the steep (zero-variance) maps produce, through eval_lean / sample_lean and the fused
    eval_leanmap / sample_leanmap kernels, against oracle.eval_lean / oracle.sample_lean: values and written-back pdfparams"""
    lc.check_map_records_against_oracle(gpu_ctx, oracle, device="cuda:0")


def test_map_records_through_the_per_hit_operators_against_the_oracle_host_arrays(gpu_ctx, oracle):
    lc.check_map_records_against_oracle(gpu_ctx, oracle)                 # host batches: the chunked pipeline in front of the same kernels
    lc.check_map_records_against_oracle(gpu_ctx, oracle, n=37)           # ... and the host twin


def _check_large_map(m, l0, first_level, n_lookups, window):
    """levels first_level .. top == pyramid_np; n_lookups hostile lookups and every texel centre of a window of level 0 == lookup_np"""
    h, w = l0.shape[:2]
    ref = lc.pyramid_np(l0)
    assert (m.width, m.height, m.levels) == (w, h, len(ref))
    for l in range(first_level, m.levels):
        got = m.level(l)
        assert got.shape == ref[l].shape and lc.same(got, ref[l]), (w, h, l, lc.first_diff(got, ref[l]))
    uv, lod = lc.hostile_coords(n_lookups, m.levels, 43)
    want = lc.lookup_np(ref, uv, lod)
    got = m.lookup(uv, lod)
    assert lc.same(got, want), (w, h, lc.first_diff(got, want))
    wh, ww = min(window, h), min(window, w)
    y0, x0 = (h - wh) // 2, (w - ww) // 3
    yy, xx = np.mgrid[y0:y0 + wh, x0:x0 + ww]
    centres = np.stack([(xx.ravel() + 0.5) / w, (yy.ravel() + 0.5) / h], 1).astype(f32)
    got = m.lookup(centres, np.zeros(len(centres), f32))
    assert lc.same(got, lc.lookup_np(ref, centres, np.zeros(len(centres), f32))), (w, h, "texel centres")


def test_large_and_extreme_map_shapes(gpu_ctx):
    """The builder, pyramid and lookup kernels at sizes where the closed form for a level's offset, 32-bit texel indices and the grid
    sizes are first exercised on the GPU (the value checks above stop at 128 x 128): from_dmap of an 8192 x 4096 random height map --
    1.4 GB of device memory --, from_moments of 8192 x 2 and 2 x 8192.  Every level from 3 up == the numpy pyramid, 2^20 hostile lookups
    and all texel centres of a 256 x 256 window of level 0 == the numpy lookup.  One map at a time."""
    rng = np.random.default_rng(8192)
    cpu = djb.cpu_context()
    d = rng.integers(0, 256, (4096, 8192), dtype=np.uint8)
    nmap = djb.dmap_to_nmap(d, 0.1, ctx=cpu)                              # the host path (held to the reference tool's bytes by test_leanmap_host.py)
    assert np.array_equal(djb.dmap_to_nmap(d, 0.1, ctx=gpu_ctx), nmap)
    m = djb.leanmap.from_dmap(d, 0.1, 1e-5, ctx=gpu_ctx)
    try:
        _check_large_map(m, lc.nmap2leanmap_np(nmap, 1e-5), 3, 1 << 20, 256)
    finally:
        m.close()
    del nmap, d
    gc.collect()
    for h, w in ((2, 8192), (8192, 2)):
        mom = (rng.standard_normal((h, w, 5)) * 3).astype(f32)
        m = djb.leanmap.from_moments(mom, ctx=gpu_ctx)
        try:
            _check_large_map(m, mom, 0, 1 << 20, 256)
        finally:
            m.close()
