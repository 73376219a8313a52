"""The cases of tests/trip_cases.py, pinned without a GPU: the trip sizes against the launch formulas, the class condition of the two queue
blocks, and the product's host path (djb.cpu_context()) against the ORACLE's bits on every block the GPU modules tile."""
import numpy as np
import pytest

import trip_cases as tc
from dj_brdf_amd import djb
from param_space_cases import in_sharp_domain, value_bits


def test_trip_sizes_follow_from_the_launch_formulas():
    """every two-trip and three-trip n launches the capped grid, and that grid times the workgroup is the trip"""
    for trips in (2, 3):
        n = tc.units("capped", trips)
        assert tc.grid_capped(n, tc.WG, tc.EVAL_GRID_CAP) * tc.WG == tc.TRIP["capped"] == 4096 * 256          # djb_kernels_eval.hip:231, 444, 794-848
        n = tc.units("aniso_eval", trips)
        assert tc.grid_aniso_eval(n) * tc.ANISO_WG == tc.TRIP["aniso_eval"] == 2048 * 1024                    # djb_kernels_eval.hip:232
        n = tc.units("sharp", trips)
        assert n >= 1 << 16 and tc.grid_sharp(n) * tc.WG == tc.TRIP["sharp"] == 4096 * 256                   # djb_kernels_eval.hip:235-239
        n = tc.units("sampler", trips)
        assert tc.grid_persistent(n) * tc.WG == tc.TRIP["sampler"] == 5120 * 256                             # djb_kernels_sample.hip:57-65, 847, 868
        n = tc.units("utia_v2", trips)
        assert tc.grid_capped(n, tc.WG, tc.UTIA_GRID_CAP) * tc.WG == tc.TRIP["utia_v2"] == 16384 * 256       # djb_kernels_utia.hip:16, 190
    for fam, trip in tc.TRIP.items():
        assert trip % tc.BLOCK_N == 0, fam                      # a later trip meets the block at the same positions
        assert tc.units(fam) % 4 == 1, fam                      # ... and the contract kernels' exact tail runs (n = 4 m + 1)
    # the workgroups of the last trip: the first 16 (4 of 1024), the last one ragged
    assert -(-(tc.BLOCK_N - tc.RAGGED) // tc.WG) == 16 and (tc.BLOCK_N - tc.RAGGED) % 64 == 13


def test_wave_counts_cover_the_four_classes():
    c = tc.WAVE_COUNTS
    assert sorted(set(tc.wave_class(x) for x in c)) == [0, 1, 2, 3]
    assert ((c >= 22) & (c <= 31)).sum() >= 4            # three trips: the residue of these drains on the third
    m = (tc.BLOCK_N - tc.RAGGED) // 64                   # whole waves of the last trip
    assert sorted(set(tc.wave_class(x) for x in c[:m])) == [0, 1, 2, 3]
    for seed in (tc.SHARP_SEED, tc.SAMPLER_SEED):
        q = tc.queued_lanes(seed).reshape(64, 64)
        assert (q.sum(1) == c).all()
        # not a prefix of the wave: the slot of a lane is its ballot prefix count
        assert any(q[w, :x].sum() != x for w, x in enumerate(c) if 0 < x < 64)


@pytest.mark.parametrize("setup", tc.SHARP_SETUPS, ids=lambda s: f"{s[0][0]}-{'shadow' if s[1] else 'noshadow'}")
def test_sharp_block_queues_exactly_the_intended_pairs(oracle, setup):
    """In every wave the number of pairs whose oracle evalp is not (+0, +0, +0) equals the intended count.  The pairs with a NaN or an infinite component
    are queued by the kernel's rule (b) (`sane` fails, o is above the horizon and i.z is not <= 0) whatever the reference returns for them: NaN with the
    Schlick term and no shadowing -- there the condition holds as it stands --, +0 in the other three set-ups, where they are counted by that rule."""
    i, o, queued = tc.sharp_block()
    odd = ~np.isfinite(i).all(1)
    assert 0 < odd.sum() <= 32 and (queued | ~odd).all() and np.isfinite(o).all()
    with np.errstate(invalid="ignore"):
        assert (o[odd, 2] > 0).all() and not (i[odd, 2] <= 0).any()
    spec = ("mf", "beckmann") + setup
    for p in tc.SHARP_LOBES:
        assert in_sharp_domain(oracle, p), p
        nz = (value_bits(tc.oracle_output(spec, "sharp", p, "evalp")) != 0).any(1)
        if setup == (tc.FRESNEL_SCHLICK, False):
            assert (nz.reshape(64, 64).sum(1) == tc.WAVE_COUNTS).all(), p
        assert ((nz | odd) == queued).all(), (p, np.flatnonzero((nz | odd) != queued)[:8])
        assert not (nz & ~queued).any()
        for op in tc.EVAL_OPS:
            tc.assert_second_trip_is_not_vacuous(f"sharp {setup} {p} {op}", tc.expected(spec, "sharp", p, op), queued)


def test_sampler_block_holds_the_deferred_families():
    u1, u2, o, deferred = tc.sampler_block()
    with np.errstate(invalid="ignore"):
        normal = (o == np.float32([0, 0, 1])).all(1)
        below = o[:, 2] < 0
        tail = (u2 <= np.float32(1e-3)) | (u2 >= np.float32(1 - 1e-3))
        nan = np.isnan(u2)
        u = 2.0 * (0.99998 * u2[tail].astype(np.float64) + 0.00001) - 1.0
    assert (-np.log(1 - u * u) > 5.0).all()                     # erfinv's tail arm: !(w < 5), with room for the float rounding (w >= 5.5)
    assert (-np.log(1 - u * u)).min() > 5.4
    for fam in (normal, below, tail, nan):
        assert fam[deferred].sum() >= 64
    assert ((normal | below | tail | nan)[deferred]).all()
    assert ((normal | below | nan) <= deferred).all()           # (a bench u2 may lie in the tail as well: 0.2 % of them)
    assert np.isfinite(u1).all() and (tail & ~deferred).sum() <= 16
    for spec in tc.SAMPLER_SPECS:
        for p in tc.SAMPLER_PARAMS:
            for op in tc.SAMPLE_OPS:
                tc.assert_second_trip_is_not_vacuous(f"sampler {p} {op}", tc.expected(spec, "sampler", p, op), deferred)


def test_second_trips_of_the_other_blocks_are_not_vacuous():
    for spec, block, plist, _, _ in tc.CAPPED.values():
        for p in plist:
            for op in tc.EVAL_OPS + tc.SAMPLE_OPS:
                tc.assert_second_trip_is_not_vacuous(f"{spec} {p} {op}", tc.expected(spec, block, p, op))
    for op in ("eval", "evalp"):
        tc.assert_second_trip_is_not_vacuous(f"utia two-tier {op}", tc.expected("utia_drawn", "finite", None, op))
    for spec, p in tc.FIXUP:
        tc.assert_second_trip_is_not_vacuous(f"fix-up {spec}", tc.expected(spec, "hostile", p, "evalp"))


@pytest.fixture(scope="module")
def cpu():
    return djb.cpu_context()


@pytest.mark.parametrize("case", tc.all_cases(), ids=tc.case_id)
def test_host_path_returns_the_oracles_bits(cpu, case):
    spec, block, p, ops = case
    b = tc.product_object(spec, cpu)
    for op in ops:
        got, want = tc.host_outputs(b, block, p, op), tc.expected(spec, block, p, op)
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape, (op, k, g.shape, w.shape)
            bad = value_bits(g) != value_bits(w)
            assert not bad.any(), f"{op} output {k}: {int(bad.sum())} values differ, first at unit {int(np.flatnonzero(bad.reshape(len(g), -1).any(1))[0])}"
