"""The HIP kernels over the PARAMETER axis: the table of tests/param_space_cases.py -- the domain edges of the sharp-lobe Beckmann kernel,
of contract mode and of its sampler, offset and fully correlated lobes, radii near both ends of the float range -- against the oracle,
which tests/test_oracle_vs_ref.py::test_parameter_space_bit_exact pins to the real reference on the same table.  On the GPU the parameters
choose the code that runs; every comparison is of value bits (signs of zeros included, NaNs as one pattern).  What makes a comparison
worth something -- enough live values, both paths of the sharp kernel fed -- is asserted from the oracle's output alone.
Also here: sgd / abc objects built from rows the caller supplies (the published rows are covered by tests/test_gpu_models.py)."""
import numpy as np
import pytest

import param_space_cases as ps
from dj_brdf_amd import djb
from test_gpu_contract import check_contract, check_directions

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dense_in(a):        # [3, n] device tensor: dense SoA views, the layout that reaches the sharp and contract kernels
    return _dev(a.T) if a.ndim == 2 else _dev(a)


def _dense_out(t):
    a = t.cpu().numpy()
    return a.T if a.ndim == 2 else a


def _strided_out(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("case", ps.CASES, ids=ps.case_id)
def test_parameter_table_on_the_device(gpu_ctx, oracle, case):
    """eval / evalp / pdf / fused eval_pdf (with and without the cosine) / sample / evalp_is of GGX and Beckmann == the oracle, bit for bit:
    dense [3, n] device batches of 2^17 + 37 pairs (the sharp kernel launches, the batch ends in a ragged wave), [n, 3] device batches, and a
    37-element host slice (answered by the host twin of the GPU object); Fresnel ideal and Schlick, inside the sharp kernel's domain also
    unpolarized and no shadowing; each set once as a plain djb_params and once in the cached form of the C++ facade's params objects
    (same bits, same status)."""
    tag, p = case
    for ndf in ("ggx", "beckmann"):
        for fres, shadow in ps.fresnels_for(oracle, p):
            ob = oracle.microfacet(ndf, fres, shadow)
            inputs = ps.pairs(oracle, ob, p)
            i, o, u1, u2 = inputs
            want = ps.oracle_outputs(oracle, ob, inputs, p)
            ps.assert_reference_side_conditions(oracle, ndf, case, want["eval"])
            g = getattr(djb, ndf)(ps.mk_fresnel(fres), shadow, ctx=gpu_ctx)
            du = (i, o, _dev(u1), _dev(u2))
            tail = tuple(a[-37:] for a in inputs)
            want_tail = {k: v[-37:] for k, v in want.items()}
            for form, up_ in (("plain", ps.mk_params(p)), ("cached", ps.mk_cached(p))):
                name = f"{ndf}/{fres[0]}/{shadow}/{p}/{form}"
                status, got = ps.product_outputs(g, du, up_, _dense_in, _dense_out)
                assert status is None, f"{name} dense: {status}"
                ps.assert_outputs_equal(name + " dense", got, want)
                status, got = ps.product_outputs(g, du, up_, _dev, _strided_out)
                assert status is None, f"{name} strided: {status}"
                ps.assert_outputs_equal(name + " strided", got, want)
                status, got = ps.product_outputs(g, tail, up_)
                assert status is None, f"{name} host slice: {status}"
                ps.assert_outputs_equal(name + " host slice", got, want_tail)


@pytest.mark.parametrize("case", ps.CASES, ids=ps.case_id)
def test_parameter_table_in_contract_mode(gpu_ctx, oracle, case):
    """DJB_OPT_CONTRACT_1E5 on, dense device batches.  A set inside the fast path's domain (ct_params: 1e-4 <= ax, ay <= 1e4, |rho| <= 0.9, no
    offset) must hold the value contract -- zeros and NaNs where the reference has them, everything else within 1e-5 relative
    (test_gpu_contract.check_contract; the 1e-5 is the project's own, BASELINE.json north_star); a set outside it -- one float outside it --
    must return the oracle's bits.  The same for sample and the sampler's domain (cts_params_ok: 1e-3 <= ax, ay <= 100, |rho| <= 0.99,
    |tx|, |ty| <= 10; directions within 1e-5 per component, test_gpu_contract.check_directions).  evalp_is keeps the reference's direction."""
    tag, p = case
    inside, inside_s = ps.in_contract_domain(oracle, p), ps.in_sample_contract_domain(oracle, p)
    djb.set_contract_1e5(gpu_ctx, True)
    try:
        for ndf in ("ggx", "beckmann"):
            for fres in (ps.FRESNEL_IDEAL, ps.FRESNEL_SCHLICK):
                ob = oracle.microfacet(ndf, fres, True)
                inputs = ps.pairs(oracle, ob, p)
                i, o, u1, u2 = inputs
                want = ps.oracle_outputs(oracle, ob, inputs, p)
                g = getattr(djb, ndf)(ps.mk_fresnel(fres), True, ctx=gpu_ctx)
                status, got = ps.product_outputs(g, (i, o, _dev(u1), _dev(u2)), ps.mk_params(p), _dense_in, _dense_out)
                name = f"contract/{ndf}/{fres[0]}/{p}"
                assert status is None, f"{name}: {status}"
                ev = {k: v for k, v in got.items() if k in ("eval", "evalp", "pdf", "fused_eval", "fused_pdf", "fused_evalp")}
                if inside:
                    for k, v in ev.items():
                        check_contract(f"{name}/{k}", v, want[ps.WANT_OF.get(k, k)])
                else:
                    ps.assert_outputs_equal(name + " (outside the domain)", ev, want)
                if inside_s:
                    check_directions(name + "/sample", got["sample"], want["sample"], o)
                else:
                    ps.assert_outputs_equal(name + " (outside the sampler's domain)", {"sample": got["sample"]}, want)
                ps.assert_outputs_equal(name, {"is_i": got["is_i"]}, want)
    finally:
        djb.set_contract_1e5(gpu_ctx, False)


def _model_rows(kind):
    return [("resampled %d" % k, r) for k, r in enumerate(ps.resampled_rows(kind))] + getattr(ps, kind + "_edge_rows")()


@pytest.mark.parametrize("kind", ["sgd", "abc"])
def test_user_supplied_model_rows(gpu_ctx, oracle, kind, monkeypatch):
    """sgd / abc objects from rows the CALLER supplies: 60 rows nobody published (every column drawn independently from the published values of
    that column, fixed seed) and rows on and over every limit of the device fast tier's domain (djb_fast_models.inc: sgd_fast_row, abc_ndf_fast).
    The fast tier -- which includes the TH_APPROX arctangent path no host tool runs -- is exhausted for the 100 published rows only; for each row here
      * from_params(row).eval on 2^16 pairs (dense device batch) == the oracle's object of the same row, in bits;
      * djb.selftest_model_fast(b, 2^22): the tier against the exact chains on the device, no mismatch;
      * sgd: the same bits from an object created with the tier off (DJB_SGD_FAST=0).
    The real reference cannot build a row (its constructors take a material name): the oracle's row path is the one pinned to it on the 100
    published rows (test_oracle_vs_ref.py::test_sgd_abc_all_materials)."""
    i, o = ps.model_pairs(1 << 16)
    di, do = _dense_in(i), _dense_in(o)
    for name, row in _model_rows(kind):
        want = oracle.eval(ps.oracle_model(oracle, kind, row), i, o)
        b = getattr(djb, kind).from_params(row, ctx=gpu_ctx)
        got = _dense_out(b.eval(di, do))
        assert np.array_equal(ps.value_bits(got), ps.value_bits(want)), (kind, name, int(np.sum(ps.value_bits(got) != ps.value_bits(want))))
        r = djb.selftest_model_fast(b, 1 << 22, seed=7, ctx=gpu_ctx)
        assert r["g1_mismatch"] == 0 and r["ndf_mismatch"] == 0, (kind, name, r)
        if kind == "sgd":
            monkeypatch.setenv("DJB_SGD_FAST", "0")
            exact = _dense_out(djb.sgd.from_params(row, ctx=gpu_ctx).eval(di, do))
            monkeypatch.delenv("DJB_SGD_FAST")
            assert np.array_equal(ps.value_bits(got), ps.value_bits(exact)), (name, "fast tier != exact chain")
