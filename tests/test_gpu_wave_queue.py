"""The extra-trip record queue (djb_worklist.hpp: recq_push / recq_drain) in its five kernels, where the other GPU tests do not take
it: a residue carried from one grid-stride trip into the next, and the last trip's partial drain at sub-tile sizes when every live
lane is queued (DJB_OPT_MERL_EXACT_ONLY).  The calls: evalp_is_proxy and evalp_pdf_proxy with a MERL target, and eval / evalp,
evalp_is_proxy and evalp_pdf_proxy of a MERL material set.

Inputs: each family's 4 096-unit block of pairs tier 1 declines (tests/merl_set_light_cases.py: declined_block for the given-pair calls;
the near-normal block of the sampling tests under the sharp isotropic(4.5e-3) GGX lobe for the sampling calls).  Expected values: the
ORACLE on that block, computed once per call and shared; compared as bits.
  second trip: the block tiled and cut to n = 1 048 576 + 4 096 - 179.  The grid is capped at 4 096 workgroups of 256 (2 048 of 512),
    1 048 576 units per trip, so 16 workgroups take a second, ragged trip with what their queues kept from the first.
  sub-tile: prefixes of the block around a wave and a 256-unit tile, exact-only: cnt < 64, cnt == 64, and the flush of a workgroup
    whose later waves are empty."""
import functools

import numpy as np
import pytest

import merl_set_cases as sets
import merl_set_light_cases as light
import proxy_is_cases as pis
import proxy_light_cases as plight
from dj_brdf_amd import djb, synth

pytestmark = pytest.mark.gpu
BLOCK_N = light.DECLINED_N                              # 4 096
TRIP = 4096 * 256                                       # units per grid-stride trip of every one of the five kernels
N_SECOND_TRIP = TRIP + BLOCK_N - 179
SUB_TILE = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)
SHARP = ("elliptic", 4.5e-3, 4.5e-3, 0.0)               # the oracle's parameters of the sharp lobe (material 2 of the set)
CALLS = ("evalp_is_proxy", "evalp_pdf_proxy", "set_eval", "set_evalp", "set_evalp_is_proxy", "set_evalp_pdf_proxy")


@pytest.fixture(scope="module")
def objects(gpu_ctx):
    members = sets.product_members(gpu_ctx)
    mset = djb.merl_set(members, sets.product_params(), ctx=gpu_ctx)
    for b in members:
        b.close()
    yield {"merl": pis.product_target("merl", gpu_ctx), "ggx": djb.ggx(ctx=gpu_ctx), "set": mset}
    mset.close()


@functools.lru_cache(maxsize=None)
def _sampler_block():
    """(ids, o, u1, u2): the near-normal block of the sampling tests at 4 096 units; every hit on material 2, every 53rd inactive"""
    o = light.near_normal_o(BLOCK_N)
    ids = np.full(BLOCK_N, 2, np.int32); ids[::53] = -1
    out = ids, o, synth.uniforms(BLOCK_N, synth.SEED_U1), synth.uniforms(BLOCK_N, synth.SEED_U2)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _case(call):
    """(inputs, want, pairs): per-unit input arrays, the oracle's outputs on them, and the (i, o) the MERL index sees (read-only)"""
    import oraclelib
    O = oraclelib.oracle()
    ids, i, o = light.declined_block()
    sids, so, u1, u2 = _sampler_block()
    if call == "evalp_is_proxy":
        want = pis.compose(O, pis.oracle_target("merl"), pis.oracle_proxy("ggx_iso"), SHARP, u1, u2, so)
        inputs, pairs = (u1, u2, so), (want[1], so)
    elif call == "evalp_pdf_proxy":
        inputs, want, pairs = (i, o), plight.expected_on(O, "merl", "ggx_iso", i, o, SHARP), (i, o)
    elif call in ("set_eval", "set_evalp"):
        per = [O.eval(om, i, o, None, call[4:]).astype(np.float32) for om in sets.oracle_materials()]
        inputs, want, pairs = (ids, i, o), (sets.select(per, ids),), (i, o)
    elif call == "set_evalp_is_proxy":
        per = pis.compose(O, sets.oracle_materials()[2], O.microfacet("ggx"), SHARP, u1, u2, so)
        want = tuple(np.where((sids == 2)[:, None] if a.ndim == 2 else sids == 2, a, np.float32(0)) for a in per)
        inputs, pairs = (sids, u1, u2, so), (per[1], so)
    else:
        inputs, want, pairs = (ids, i, o), light.expected_on("ggx", ids, i, o), (i, o)
    want = tuple(np.asarray(a, np.float32) for a in want)
    for a in want:
        a.setflags(write=False)
    return inputs, want, pairs


def _tiled(a, n):
    """the block repeated and cut to n units"""
    return np.concatenate([a] * -(-n // len(a)))[:n]


def _run(objects, call, inputs, layout):
    """one device call; vec3 batches [3, n] (dense) or [n, 3] (strided) -> the outputs as numpy, vec3 as [n, 3]"""
    import torch
    dev = f"cuda:{objects['set'].ctx.device}"

    def put(a):
        if a.ndim == 2:
            a = a if layout == "strided" else a.T
        return torch.from_numpy(np.array(a, order="C")).to(dev)           # a copy: the cases are read-only
    args = [put(a) for a in inputs]
    ggx, sharp = objects["ggx"], djb.microfacet.params.isotropic(4.5e-3)
    if call == "evalp_is_proxy":
        out = objects["merl"].evalp_is_proxy(ggx, *args, None, sharp)
    elif call == "evalp_pdf_proxy":
        out = objects["merl"].evalp_pdf_proxy(ggx, *args, None, sharp)
    elif call == "set_eval":
        out = (objects["set"].eval(*args),)
    elif call == "set_evalp":
        out = (objects["set"].evalp(*args),)
    else:
        out = getattr(objects["set"], call[4:])(ggx, *args)
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in out]
    return [a.T if a.ndim == 2 and layout == "dense" else a for a in out]


def _assert_same(tag, got, want):
    assert len(got) == len(want), (tag, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (tag, k, g.shape, w.shape)
        ok = pis.same_bits(g, w)
        if not ok.all():
            bad = np.argwhere(~ok)
            at = tuple(bad[0])
            raise AssertionError(f"{tag}: output {k} differs in {len(bad)} of {ok.size} values, first at {at}: got {g[at]!r} want {w[at]!r}")


def _assert_block_is_declined(gpu_ctx, call):
    """a condition on the inputs: the block's pairs reach the lanes tier 1 decides and, by at least a wave, the ones it declines"""
    import torch
    i, o = _case(call)[2]
    with np.errstate(invalid="ignore"):
        live = i[:, 2] > 0
    dev = f"cuda:{gpu_ctx.device}"
    stats = djb.merl_guard_stats(torch.from_numpy(np.ascontiguousarray(i[live].T)).to(dev), torch.from_numpy(np.ascontiguousarray(o[live].T)).to(dev), ctx=gpu_ctx)
    print(f"merl_guard_stats on the block of {call}:", stats)
    assert stats["ambiguous"] + stats["special"] >= 64 and stats["certain"] > 0 and stats["mismatch"] == 0, stats


@pytest.mark.parametrize("call", CALLS)
def test_a_residue_is_carried_into_the_second_trip(gpu_ctx, objects, call):
    _assert_block_is_declined(gpu_ctx, call)
    inputs, want, _ = _case(call)
    n = N_SECOND_TRIP
    big_in, big_want = [_tiled(a, n) for a in inputs], [_tiled(a, n) for a in want]
    for exact in (False, True):
        djb.set_merl_exact_only(gpu_ctx, exact)
        try:
            for layout in ("dense", "strided"):
                _assert_same(f"{call}, {layout}, n = {n}, exact only = {exact}", _run(objects, call, big_in, layout), big_want)
        finally:
            djb.set_merl_exact_only(gpu_ctx, False)


@pytest.mark.parametrize("call", CALLS)
def test_sub_tile_sizes_with_every_live_lane_queued(gpu_ctx, objects, call):
    _assert_block_is_declined(gpu_ctx, call)
    inputs, want, _ = _case(call)
    djb.set_merl_exact_only(gpu_ctx, True)
    try:
        for n in SUB_TILE:
            for layout in ("dense", "strided"):
                _assert_same(f"{call}, {layout}, n = {n}, exact only", _run(objects, call, [a[:n] for a in inputs], layout), [a[:n] for a in want])
    finally:
        djb.set_merl_exact_only(gpu_ctx, False)
