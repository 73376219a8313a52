"""The light-sample call on the host path (CPU context): brdf.evalp_pdf_proxy / djb_evalp_pdf_proxy_batch against the oracle's separate
evalp and proxy pdf, guarded as the plugins guard them (tests/proxy_light_cases.py); layouts, the facade members, a user_brdf target,
the error cases of the C ABI.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import proxy_light_cases as cases
from dj_brdf_amd import _lib, djb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dj_brdf_amd", "lib")
SIZES = (1, 2, 97)
OK, INVALID = 0, 1


@pytest.fixture(scope="module")
def cpu():
    return djb.cpu_context()


@pytest.fixture(scope="module")
def objects(cpu):
    """the product's objects on the CPU context, built once"""
    cache = {}

    def get(role, name):
        key = (role, cases.PROXIES[name][0] if name in cases.PROXIES else name)
        if key not in cache:
            cache[key] = (cases.product_target if role == "target" else cases.product_proxy)(name, cpu)
        return cache[key]
    return get


def test_inputs_exercise_every_class():
    cases.assert_input_conditions()


@pytest.mark.parametrize("target,proxy", cases.GPU_PAIRS, ids=lambda v: v)
def test_cpu_context_equals_the_oracle(objects, target, proxy):
    i, o = cases.inputs()
    want = cases.expected(target, proxy)
    t, p, pp = objects("target", target), objects("proxy", proxy), cases.product_params(proxy)
    for n in (cases.N,) + SIZES:
        got = t.evalp_pdf_proxy(p, i[:n], o[:n], None, pp)
        assert got[0].shape == (n, 3) and got[1].shape == (n,)
        cases.assert_same(f"{target} <- {proxy}, n = {n}", got, [a[:n] for a in want], target, i[:n], o[:n])
    # the guarded pairs are +0 bits
    fr, pdf = (np.asarray(a) for a in t.evalp_pdf_proxy(p, i, o, None, pp))
    z = cases.guarded(i, o)
    assert not fr[z].view(np.uint32).any() and not pdf[z].view(np.uint32).any()


def test_lambert_as_target_and_as_proxy(objects, oracle):
    """the host path serves every pair of kinds"""
    i, o = cases.inputs()
    lam = objects("target", "lambert")
    refl = (0.8, 0.5, 0.25)
    want = cases.expected_on(oracle, "lambert", "ggx_ell", i, o, target_params=("lambert",) + refl)
    got = lam.evalp_pdf_proxy(objects("proxy", "ggx_ell"), i, o, djb.lambert.params(refl), cases.product_params("ggx_ell"))
    cases.assert_same("lambert <- ggx", got, want)
    assert np.nansum(np.abs(want[0])) > 0
    want = cases.expected_on(oracle, "abc", "lambert", i, o)
    cases.assert_same("abc <- lambert", objects("target", "abc").evalp_pdf_proxy(lam, i, o), want)
    assert (want[1] > 0).sum() > cases.N // 2


@pytest.mark.parametrize("target,proxy", (("merl", "ggx_ell"), ("sgd", "tabular"), ("utia", "beckmann_iso")), ids=lambda v: v)
def test_strided_and_soa_views(objects, target, proxy):
    i, o = cases.inputs()
    n = 4001
    want = [a[:n] for a in cases.expected(target, proxy)]
    t, p, pp = objects("target", target), objects("proxy", proxy), cases.product_params(proxy)
    cases.assert_same("aos", t.evalp_pdf_proxy(p, i[:n], o[:n], None, pp), want, target, i[:n], o[:n])                 # [n, 3]: stride 3
    fr, pdf = t.evalp_pdf_proxy(p, np.ascontiguousarray(i[:n].T), np.ascontiguousarray(o[:n].T), None, pp)
    assert fr.shape == (3, n)
    cases.assert_same("soa", (fr.T, pdf), want, target, i[:n], o[:n])                                                 # [3, n]: stride 1


FACADE_O = np.float32([[0.1, 0.3, 0.9486833], [0.3, 0.2, 0.9327379], [0.5, 0.1, 0.8602325], [0.7, 0.0, 0.7141428], [0.9, -0.1, -0.4242641]])
FACADE_I = np.float32([[-0.1, -0.25, 0.9630680], [-0.3, -0.2, -0.9327379], [0.1, 0.5, 0.8602325], [-0.6, 0.1, 0.7937254], [0.2, 0.2, 0.9591663]])


def test_facade_members_equal_the_python_mirror(objects, tmp_path):
    src = os.path.join(ROOT, "tests", "api", "proxy_light_facade.cpp")
    exe = tmp_path / "proxy_light_facade"
    r = subprocess.run(["g++", "-O1", "-std=c++14", "-DNVERBOSE", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), src, "-L" + LIBDIR, "-ldjb_hip",
                        "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], env=dict(os.environ, DJB_DEVICE="cpu", DJB_QUIET="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = {}
    for line in out.stdout.splitlines():
        tag, *vals = line.split()
        rows.setdefault(tag, []).append([float.fromhex(v) for v in vals])
    for tag, target, proxy in (("abc_ggx", "abc", "ggx_ell"), ("sgd_beckmann", "sgd", "beckmann_iso")):
        fr, pdf = objects("target", target).evalp_pdf_proxy(objects("proxy", proxy), FACADE_I, FACADE_O, None, cases.product_params(proxy))
        assert np.abs(fr[[0, 2, 3]]).sum(1).all() and (pdf[[0, 2, 3]] > 0).all()                  # three live pairs
        assert not fr[[1, 4]].view(np.uint32).any() and not pdf[[1, 4]].view(np.uint32).any()     # i.z < 0, o.z < 0
        want = np.concatenate([fr, pdf[:, None]], 1).astype(np.float32)
        for form in ("scalar", "batch"):
            got = np.float32(rows[f"{tag}_{form}"])
            assert got.shape == want.shape and cases.same_bits(got, want).all(), (tag, form, got, want)


def test_a_user_brdf_target_gets_the_composed_values(cpu, objects, oracle):
    """host code on the target side: the object's own evalp, the proxy's pdf, the guard applied last"""
    lobe = ("phong", 0.05, 0.04, 0.03, 0.9, 0.8, 0.7, 50.0)
    oc = oracle.custom(*lobe)

    class phong(djb.user_brdf):
        def eval(self, i, o, user_param=None):
            return oracle.eval(oc, i, o)
    i, o = (a[:8001] for a in cases.inputs())
    z = cases.guarded(i, o)
    t, p, pp = phong(ctx=cpu), objects("proxy", "ggx_ell"), cases.product_params("ggx_ell")
    fr, pdf = t.evalp_pdf_proxy(p, i, o, None, pp)
    with np.errstate(all="ignore"):
        wfr = np.array(t.evalp(i, o), np.float32).reshape(-1, 3)
    wfr[z] = 0
    wpdf = cases.oracle_pdf(oracle, "ggx_ell", i, o, cases.oracle_params("ggx_ell"))
    assert cases.same_bits(fr, wfr).all() and cases.same_bits(pdf, wpdf).all()
    assert not fr[z].view(np.uint32).any() and not pdf[z].view(np.uint32).any() and np.nansum(np.abs(fr[~z])) > 0


# ------------------------------------------------------------------ the C ABI's error cases
def _call(ctx, target, proxy, n=4, fr=True, pdf=True):
    lib = _lib.load()
    d = np.tile(np.float32([[0.3, 0.1, 0.9]]), (max(n, 1), 1))
    out, opdf = np.full((max(n, 1), 3), 7, np.float32), np.full(max(n, 1), 7, np.float32)
    vd, vout = djb._Vec(d), djb._Vec(out)
    st = lib.djb_evalp_pdf_proxy_batch(ctx._h, target._h if target is not None else None, proxy._h if proxy is not None else None, C.c_int64(n),
                                       C.byref(vd.view), C.byref(vd.view), None, None, C.byref(vout.view) if fr else None,
                                       C.c_void_p(opdf.ctypes.data) if pdf else None, C.c_int(_lib.MEM_HOST))
    return st, lib.djb_last_error().decode(errors="replace"), out, opdf


def test_error_cases(objects, cpu):
    abc, ggx = objects("target", "abc"), objects("proxy", "ggx_iso")
    st, msg, out, opdf = _call(cpu, abc, ggx, fr=False)
    assert st == INVALID and "out_fr" in msg and (opdf == 7).all(), (st, msg)
    st, msg, out, opdf = _call(cpu, abc, ggx, pdf=False)
    assert st == INVALID and "out_pdf" in msg and (out == 7).all(), (st, msg)
    st, msg, out, opdf = _call(cpu, None, ggx)
    assert st == INVALID and "null brdf" in msg and "target" in msg and (out == 7).all() and (opdf == 7).all(), (st, msg)
    st, msg, out, opdf = _call(cpu, abc, None)
    assert st == INVALID and "null brdf" in msg and "proxy" in msg and (out == 7).all() and (opdf == 7).all(), (st, msg)
    other = djb.Context("cpu")
    st, msg, out, opdf = _call(cpu, abc, djb.ggx(ctx=other))
    assert st == INVALID and "different contexts" in msg and (out == 7).all() and (opdf == 7).all(), (st, msg)
    st, msg, out, opdf = _call(cpu, abc, ggx, n=0)
    assert st == OK and (out == 7).all() and (opdf == 7).all(), (st, msg)
    st, msg, out, opdf = _call(cpu, abc, ggx)
    assert st == OK and (opdf > 0).all() and (out > 0).all(), (st, msg, out, opdf)
    with pytest.raises(djb.exc):
        abc.evalp_pdf_proxy(djb.ggx(ctx=other), np.float32([[0, 0, 1]]), np.float32([[0, 0, 1]]))
