"""VALUES where tests/test_gpu_bounds.py checks only writes: the ten objects of its `_objects`, with their parameter sets, and every batch operator of
the C ABI (sample_rng included) on device memory at sizes below / across the 4-pair, wave and workgroup granularities of the kernels, in five placements:
  aligned     dense planes, every array 16-byte aligned
  misaligned  dense planes, i, o, u1, u2 and the outputs each starting 1-3 floats off a 16-byte boundary
  aos3        [n, 3] records
  aos4        padded float4 records (stride 4; the fourth float must stay untouched)
  mixed       i dense, o [n, 3], outputs stride 4
A kernel whose ragged tail or misaligned dense path (lane_byte_offset / dense_off) returned its neighbour's value would pass the bounds test; here every unit
of every prefix of the 4 096-unit blocks of tests/trip_cases.py is held against the ORACLE's result for that unit (units are independent: a prefix has the
prefix's results) -- its bits in exact mode, the contract of tests/test_gpu_contract.py (check_contract / check_directions; the sampled direction of evalp_is
stays bit-exact) under DJB_OPT_CONTRACT_1E5.  sample_rng is compared with the array path fed by gen_uniforms at the same seeds and start.  Outputs lie between
sentinels as in tests/trip_cases.Arr: every unit written, nothing else."""
import numpy as np
import pytest

import trip_cases as tc
from dj_brdf_amd import djb, synth
from param_space_cases import mk_params
from test_gpu_contract import check_contract, check_directions

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095)
VEC, ALL = ("i", "o", "out", "w"), ("i", "o", "u1", "u2", "out", "w", "pdf")
PLACEMENTS = {
    "aligned": ({}, {}),
    "misaligned": ({}, {"i": 1, "o": 2, "u1": 3, "u2": 2, "out": 3, "w": 1, "pdf": 2}),
    "aos3": ({k: "aos3" for k in VEC}, {}),
    "aos4": ({k: "aos4" for k in VEC}, {}),
    "mixed": ({"i": "dense", "o": "aos3", "out": "aos4", "w": "aos4"}, {}),
}
RNG = (5, 6, 17)        # seed_u1, seed_u2, start


@pytest.fixture(scope="module")
def objects(gpu_ctx):
    return {name: tc.product_object(spec, gpu_ctx) for name, (spec, _, _) in tc.BATCH_OBJECTS.items()}


@pytest.fixture(scope="module")
def blocks(gpu_ctx):
    import torch
    dev = tc.device_of(gpu_ctx)
    return {block: dict(zip(("i", "o", "u1", "u2"), (tc.upload(torch, dev, a) for a in tc.BLOCKS[block]()))) for block in ("hostile", "finite")}


@pytest.mark.parametrize("contract", [False, True], ids=["exact", "contract"])
@pytest.mark.parametrize("name", list(tc.BATCH_OBJECTS))
def test_batch_operators_return_the_oracles_values(gpu_ctx, objects, blocks, name, contract):
    import torch
    dev = tc.device_of(gpu_ctx)
    spec, block, p = tc.BATCH_OBJECTS[name]
    b, up = objects[name], mk_params(p) if p is not None else None
    want = {op: tc.expected(spec, block, p, op) for op in tc.OPS}
    want_dev = {op: tuple(tc.upload(torch, dev, tc.bits_i32(a)) for a in w) for op, w in want.items()}
    o_host = tc.BLOCKS[block]()[1]
    gu1, gu2 = djb.gen_uniforms(tc.BLOCK_N, RNG[0], RNG[2], ctx=gpu_ctx), djb.gen_uniforms(tc.BLOCK_N, RNG[1], RNG[2], ctx=gpu_ctx)
    worst = 0.0
    djb.set_contract_1e5(gpu_ctx, contract)
    try:
        for n in SIZES:
            src = {k: t[:n] for k, t in blocks[block].items()}
            for pname, (lay, off) in PLACEMENTS.items():
                for op in tc.OPS:
                    tag = f"{name}, {op}, n = {n}, {pname}, contract = {contract}"
                    ins, outs = tc.call(gpu_ctx, b, op, n, src, up, torch, dev, layouts=lay, offs=off)
                    for k, (out, wd, wh) in enumerate(zip(outs, want_dev[op], want[op])):
                        if not contract or tc.OPS[op][k] == "is_i":
                            out.check_bits(f"{tag}, output {k}", wd[:n])
                            continue
                        out.check_frame(f"{tag}, output {k}")
                        if op == "sample":
                            worst = max(worst, check_directions(f"{tag}", out.values(), wh[:n], o_host[:n]))
                        else:
                            worst = max(worst, check_contract(f"{tag}, output {k}", out.values(), wh[:n]))
                    tc.check_inputs_unchanged(tag, ins, src)
                # sample_rng against the array path fed with the generator's uniforms
                rsrc = {"o": src["o"], "u1": gu1[:n], "u2": gu2[:n]}
                _, (ref,) = tc.call(gpu_ctx, b, "sample", n, rsrc, up, torch, dev, layouts=lay, offs=off)
                _, (got,) = tc.call(gpu_ctx, b, "sample", n, rsrc, up, torch, dev, layouts=lay, offs=off, rng=RNG)
                tag = f"{name}, sample_rng, n = {n}, {pname}, contract = {contract}"
                ref.check_frame(tag + " (array path)")
                if contract:
                    got.check_frame(tag)
                    check_directions(tag, got.values().reshape(n, 3), ref.values().reshape(n, 3), o_host[:n])
                else:
                    got.check_bits(tag, ref.values_bits()[1])
    finally:
        djb.set_contract_1e5(gpu_ctx, False)
    if contract:
        print(f"{name}: worst difference under the contract {worst:.3e}")


def test_the_generator_feeds_sample_rng(gpu_ctx):
    """the uniforms the comparison above feeds the array path with are the ones sample_rng draws: synth.rng_uniforms at the same seed and start"""
    for seed in RNG[:2]:
        u = djb.gen_uniforms(tc.BLOCK_N, seed, RNG[2], ctx=gpu_ctx).cpu().numpy()
        assert np.array_equal(u.view(np.uint32), synth.rng_uniforms(tc.BLOCK_N, seed, RNG[2]).view(np.uint32))
