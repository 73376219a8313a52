"""The two per-hit proxy steps of a scene on the host path (CPU context): djb.scene.evalp_is_proxy / .evalp_pdf_proxy against the oracle's
per-slot results selected by scene id (tests/scene_proxy_cases.py) -- both lobes, the 18-slot scene, the permuted table, scenes with fewer
member sets, a model-only scene without a lobe --, the proxy parameters of a UTIA set, and the refusals of the C ABI.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import merl_set_cases
import model_set_cases
import scene_proxy_cases as cases
import utia_set_cases
from dj_brdf_amd import _lib, djb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dj_brdf_amd", "lib")
INVALID = cases.INVALID


@pytest.fixture(scope="module")
def cpu():
    return djb.cpu_context()


def _members(ctx, prepared=True):
    out = {}
    src = merl_set_cases.product_members(ctx)
    out["merl"] = djb.merl_set(src, ctx=ctx)
    for b in src:
        b.close()
    src = utia_set_cases.product_members(ctx)
    out["utia"] = djb.utia_set(src, ctx=ctx)
    for b in src:
        b.close()
    for kind in model_set_cases.KINDS:
        out[kind] = djb.model_set.from_rows(kind, model_set_cases.rows(kind), ctx=ctx)
    if prepared:
        cases.prepare_members(out)
    return out


@pytest.fixture(scope="module")
def members(cpu):
    out = _members(cpu)
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(scope="module")
def main(cpu, members):
    s = djb.scene(slots=cases.TABLE, ctx=cpu, **members)
    yield s
    s.close()


@pytest.fixture(scope="module")
def lobes(cpu):
    return {"ggx": djb.ggx(ctx=cpu), "beckmann": djb.beckmann(ctx=cpu)}


def test_inputs_are_what_the_cases_say():
    cases.assert_input_conditions()


@pytest.mark.parametrize("pk", cases.PROXY_KINDS)
def test_sampling_equals_the_oracle_selection(main, lobes, pk):
    ids = cases.material_ids()
    o, u1, u2 = cases.sampler_inputs()
    want = cases.expected_sample(pk)
    mask = cases.compared_sample(ids, cases.TABLE, want[1], o)
    for n in (cases.N, 1, 2, 97):
        got = main.evalp_is_proxy(lobes[pk], ids[:n], u1[:n], u2[:n], o[:n])
        cases.assert_sample(f"{pk}, sampling, n = {n}", got, cases.head(want, n), mask[:n])


@pytest.mark.parametrize("pk", cases.PROXY_KINDS)
def test_light_sample_equals_the_oracle_selection(main, lobes, pk):
    ids = cases.material_ids()
    i, o = cases.light_inputs()
    want = cases.expected_light(pk)
    mask = cases.compared_light(ids, cases.TABLE, i, o)
    for n in (cases.N, 1, 2, 97):
        got = main.evalp_pdf_proxy(lobes[pk], ids[:n], i[:n], o[:n])
        cases.assert_light(f"{pk}, light sample, n = {n}", got, cases.head(want, n), mask[:n])


def test_the_permuted_table(cpu, members, main, lobes):
    """same members, other slot order, a slot without material and an alias: the ids mean something else"""
    s = djb.scene(slots=cases.TABLE2, ctx=cpu, **members)
    try:
        ids = cases.material_ids(len(cases.TABLE2))
        o, u1, u2 = cases.sampler_inputs()
        i, lo = cases.light_inputs()
        want_s, want_l = cases.expected_sample("ggx", cases.TABLE2), cases.expected_light("ggx", cases.TABLE2)
        mask_s, mask_l = cases.compared_sample(ids, cases.TABLE2, want_s[1], o), cases.compared_light(ids, cases.TABLE2, i, lo)
        got_s, got_l = s.evalp_is_proxy(lobes["ggx"], ids, u1, u2, o), s.evalp_pdf_proxy(lobes["ggx"], ids, i, lo)
        cases.assert_sample("table 2, sampling", got_s, want_s, mask_s)
        cases.assert_light("table 2, light sample", got_l, want_l, mask_l)
        none = ids == cases.TABLE2.index(None)
        assert none.sum() > 1000 and not any(np.asarray(a)[none].view(np.uint32).any() for a in got_s + got_l)
        # the main table on these ids gives another result: the table is what decides
        assert cases.differs(main.evalp_is_proxy(lobes["ggx"], ids, u1, u2, o), want_s, mask_s)
        assert cases.differs(main.evalp_pdf_proxy(lobes["ggx"], ids, i, lo), want_l, mask_l)
    finally:
        s.close()


@pytest.mark.parametrize("kinds", [("abc",), ("sgd", "abc"), ("merl", "sgd"), ("utia", "sgd", "abc")])
def test_scenes_with_fewer_member_sets(cpu, members, lobes, kinds):
    """a model-only scene takes proxy=None; any scene ignores the kinds it has no set for"""
    table = cases.table_without([k for k in cases.KINDS if k not in kinds])
    s = djb.scene(slots=table, ctx=cpu, **{k: members[k] for k in kinds})
    try:
        n = 8001
        ids = cases.material_ids()[:n]
        o, u1, u2 = cases.head(cases.sampler_inputs(), n)
        i, lo = cases.head(cases.light_inputs(), n)
        lobe = None if set(kinds) <= {"sgd", "abc"} else lobes["beckmann"]
        want = cases.expected_sample_on("beckmann", ids, table, o, u1, u2)
        cases.assert_sample(f"members {kinds}, sampling", s.evalp_is_proxy(lobe, ids, u1, u2, o), want, cases.compared_sample(ids, table, want[1], o))
        cases.assert_light(f"members {kinds}, light sample", s.evalp_pdf_proxy(lobe, ids, i, lo), cases.expected_light_on("beckmann", ids, table, i, lo),
                           cases.compared_light(ids, table, i, lo))
        assert (np.nan_to_num(want[2]) > 0).sum() > n // 20
    finally:
        s.close()


def test_utia_set_parameters(cpu, lobes):
    """set, info, replace; a replacement after the scene was built is what the next call sees"""
    src = utia_set_cases.product_members(cpu)
    u = djb.utia_set(src, ctx=cpu)
    s = djb.scene(utia=u, slots=[("utia", m) for m in range(3)], ctx=cpu)
    try:
        assert u.has_proxy_params is False and u.n_materials == 3
        n = 4001
        ids = (np.arange(n) % 3).astype(np.int32)
        o, u1, u2 = cases.head(cases.sampler_inputs(), n)
        table = tuple(("utia", m) for m in range(3))
        with pytest.raises(djb.exc) as e:
            s.evalp_is_proxy(lobes["ggx"], ids, u1, u2, o)
        assert e.value.status == INVALID and "utia member" in str(e.value) and "no proxy parameters" in str(e.value)
        P = djb.microfacet.params
        u.set_proxy_params([P.isotropic(0.5)] * 3)
        assert u.has_proxy_params is True
        first = s.evalp_is_proxy(lobes["ggx"], ids, u1, u2, o)
        u.set_proxy_params(cases.utia_product_params())
        want = cases.expected_sample_on("ggx", ids, table, o, u1, u2)
        mask = cases.compared_sample(ids, table, want[1], o)
        got = s.evalp_is_proxy(lobes["ggx"], ids, u1, u2, o)
        cases.assert_sample("after the replacement", got, want, mask)
        assert cases.differs(first, want, mask)
        for bad in ([P.isotropic(0.5)] * 2, None):
            with pytest.raises(djb.exc):
                u.set_proxy_params(bad)
        lib = _lib.load()
        assert lib.djb_utia_set_set_proxy_params(None, None) == INVALID and "null utia set" in lib.djb_last_error().decode()
        assert lib.djb_utia_set_set_proxy_params(u._h, None) == INVALID and "null proxy_params" in lib.djb_last_error().decode()
        assert lib.djb_utia_set_proxy_info(None, None) == INVALID and lib.djb_utia_set_proxy_info(u._h, None) == 0
        follows = (_lib.Params * 3)(*[p._p for p in cases.utia_product_params()])
        follows[1].kind |= 0x100                                       # DJB_PARAMS_RESOLVED_FOLLOWS
        assert lib.djb_utia_set_set_proxy_params(u._h, follows) == INVALID and "RESOLVED_FOLLOWS" in lib.djb_last_error().decode()
        cases.assert_sample("after the refused replacements", s.evalp_is_proxy(lobes["ggx"], ids, u1, u2, o), want, mask)
        ab, ag = u.fit_proxies(16, False)                              # as merl_set.fit_proxies: one batched fit, installed per material
        assert ab.shape == ag.shape == (3,) and np.isfinite(ag).all() and (ag > 0).all() and u.has_proxy_params
        assert cases.differs(s.evalp_is_proxy(lobes["ggx"], ids, u1, u2, o), want, mask)
    finally:
        s.close(); u.close()
        for b in src:
            b.close()


def test_facade_class_equals_the_members_own_calls(tmp_path):
    src = os.path.join(ROOT, "tests", "api", "scene_proxy_facade.cpp")
    exe = tmp_path / "scene_proxy_facade"
    r = subprocess.run(["g++", "-O1", "-std=c++14", "-DNVERBOSE", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), src, "-L" + LIBDIR, "-ldjb_hip",
                        "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], env=dict(os.environ, DJB_DEVICE="cpu", DJB_QUIET="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hits checked" in out.stdout and " 0 differ" in out.stdout, out.stdout


# ------------------------------------------------------------------ the C ABI's refusals
def test_refusals(cpu, main, members, lobes):
    other = djb.Context("cpu")
    other_lobe = djb.ggx(ctx=other)
    try:
        cases.assert_refusals(cpu, main, members, lobes, other, other_lobe, _members)
    finally:
        other_lobe.close(); other.close()
