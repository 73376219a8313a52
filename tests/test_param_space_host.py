"""The product's HOST path (the CPU context) over the parameter table of tests/param_space_cases.py, against the oracle -- which
tests/test_oracle_vs_ref.py::test_parameter_space_bit_exact pins to the real reference on the same table.  Every value bit (signs of
zeros included, NaNs as one pattern); each set once as a plain djb_params and once in the cached form of the C++ facade's params
objects.  tests/test_gpu_param_space.py runs the same table through the HIP kernels."""
import numpy as np
import pytest

import param_space_cases as ps
from dj_brdf_amd import djb

N_HOST = (1 << 14) + 37


@pytest.mark.parametrize("case", ps.CASES, ids=ps.case_id)
def test_host_path_over_the_parameter_table(oracle, case):
    """eval / evalp / pdf / fused eval_pdf / sample / evalp_is of GGX and Beckmann on the CPU context == the oracle, bit for bit, for the
    plain and the cached parameter form (same bits, same status).  Asserted first, from the oracle's output alone: a `regular` case has
    at least LIVE_FLOOR finite non-zero eval values, a Beckmann batch inside the sharp kernel's domain holds SHARP_ZERO_SHARE all-zero
    results."""
    tag, p = case
    ctx = djb.cpu_context()
    for ndf in ("ggx", "beckmann"):
        for fres, shadow in ps.fresnels_for(oracle, p):
            ob = oracle.microfacet(ndf, fres, shadow)
            inputs = ps.pairs(oracle, ob, p, N_HOST)
            want = ps.oracle_outputs(oracle, ob, inputs, p)
            ps.assert_reference_side_conditions(oracle, ndf, case, want["eval"])
            g = getattr(djb, ndf)(ps.mk_fresnel(fres), shadow, ctx=ctx)
            for form, up_ in (("plain", ps.mk_params(p)), ("cached", ps.mk_cached(p))):
                status, got = ps.product_outputs(g, inputs, up_)
                assert status is None, f"{ndf} {p} {form}: {status}"
                ps.assert_outputs_equal(f"{ndf}/{fres[0]}/{shadow}/{p}/{form}", got, want)


@pytest.mark.parametrize("kind", ["sgd", "abc"])
def test_host_path_user_supplied_model_rows(oracle, kind):
    """sgd / abc objects built from rows nobody published (every column resampled from the published values of that column) and from rows
    on the edges of the device fast tier's domain: from_params(row).eval on the CPU context == the oracle's object of the same row.  The real
    reference cannot build a row (its constructors take a material name); the oracle's row path is the one pinned to it on the 100 published
    rows (test_oracle_vs_ref.py::test_sgd_abc_all_materials)."""
    i, o = ps.model_pairs(1 << 13)
    h = i.copy()
    h[::3, :2] *= np.float32(1e-3); h[::3, 2] = 1.0; h[::3] /= np.linalg.norm(h[::3], axis=1, keepdims=True)      # a third next to the normal
    ctx = djb.cpu_context()
    rows = [("resampled %d" % k, r) for k, r in enumerate(ps.resampled_rows(kind))] + getattr(ps, kind + "_edge_rows")()
    for name, row in rows:
        want = oracle.eval(ps.oracle_model(oracle, kind, row), i, o)
        b = getattr(djb, kind).from_params(row, ctx=ctx)
        got = b.eval(i, o)
        assert np.array_equal(ps.value_bits(got), ps.value_bits(want)), (kind, name, int(np.sum(ps.value_bits(got) != ps.value_bits(want))))
        # the terms on their own: eval's diffuse part absorbs a lobe of -0 (signs of zeros count)
        ob = ps.oracle_model(oracle, kind, row)
        for which, got in [("ndf", b.ndf(h))] + ([("g1", b.g1(h))] if kind == "sgd" else []):
            want = oracle.model_query(ob, which, h)
            assert np.array_equal(ps.value_bits(got), ps.value_bits(want)), (kind, name, which, int(np.sum(ps.value_bits(got) != ps.value_bits(want))))
