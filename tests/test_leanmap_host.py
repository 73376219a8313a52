"""Resident LEAN maps on the CPU context (runs without a GPU): level 0 against the real reference's fixtures, the pyramid and the
trilinear lookup against the numpy restatement of include/djb_hip.h, the fused per-hit calls against the composed ones, the
property LEAN filtering exists for, errors and lifetime.  tests/test_gpu_leanmap.py runs the same checks on the MI355X."""
import numpy as np
import pytest

import leanmap_cases as lc
from dj_brdf_amd import djb


@pytest.fixture(scope="module")
def ctx():
    return djb.cpu_context()


def test_level0_is_the_reference_tools_output(ctx):
    lc.check_level0_against_reference(ctx)


def test_moments_import_and_bias(ctx):
    lc.check_moments_import_and_bias(ctx)


def test_pyramid_and_lookup_match_the_definition(ctx):
    lc.check_pyramid_and_lookup(ctx)


def test_level_offsets_of_every_shape(ctx):
    """the closed form the kernels use for where a level starts, against plain accumulation: a map whose texels are their own
    index reads back level by level in order (all 14 x 14 shapes up to 64 x 64 and the non-square extremes)"""
    shapes = [(1 << a, 1 << b) for a in range(7) for b in range(7)] + [(8192, 1), (1, 8192), (2048, 2)]
    for w, h in shapes:
        mom = np.zeros((h, w, 5), np.float32)
        mom[..., 0] = np.arange(w * h, dtype=np.float32).reshape(h, w)
        m = djb.leanmap.from_moments(mom, ctx=ctx)
        ref = lc.pyramid_np(mom)
        assert m.levels == len(ref) == 1 + max(w, h).bit_length() - 1
        for l in range(m.levels):
            assert lc.same(m.level(l), ref[l]), (w, h, l)


def test_fused_calls_equal_lookup_then_lean(ctx):
    lc.check_fused_equals_composed(ctx, sizes=(37, 5000))


def test_filtered_moments_widen_the_lobe(ctx):
    lc.check_lean_property(ctx)


def test_errors_and_lifetime(ctx):
    lc.check_errors(ctx)


def test_map_records_through_the_per_hit_operators_against_the_oracle(ctx, oracle):
    lc.check_map_records_against_oracle(ctx, oracle)
