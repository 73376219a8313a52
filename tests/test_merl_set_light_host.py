"""The light-sample call of MERL material sets on the host path (CPU context): djb.merl_set.evalp_pdf_proxy /
djb_merl_set_evalp_pdf_proxy_batch against the oracle's per-material evalp and proxy pdf, guarded as dj_merl guards them and selected by
id (tests/merl_set_light_cases.py); layouts, the facade class, the error cases of the C ABI.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import merl_set_light_cases as cases
from dj_brdf_amd import _lib, djb, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dj_brdf_amd", "lib")
SIZES = (1, 2, 97)
OK, INVALID, NOT_IMPLEMENTED = 0, 1, 5
KINDS = ("ggx", "beckmann")


@pytest.fixture(scope="module")
def cpu():
    return djb.cpu_context()


@pytest.fixture(scope="module")
def mset(cpu):
    """the three-material set; its sources are destroyed before the first call"""
    members = cases.product_members(cpu)
    s = djb.merl_set(members, cases.product_params(), ctx=cpu)
    for b in members:
        b.close()
    yield s
    s.close()


@pytest.fixture(scope="module")
def proxies(cpu):
    return {"ggx": djb.ggx(ctx=cpu), "beckmann": djb.beckmann(ctx=cpu)}


def test_inputs_exercise_every_class():
    cases.assert_input_conditions()


@pytest.mark.parametrize("proxy", KINDS)
def test_equals_the_oracle_selection(mset, proxies, proxy):
    ids, _ = cases.material_ids()
    i, o = cases.inputs()
    want = cases.expected(proxy)
    for n in (cases.N,) + SIZES:
        got = mset.evalp_pdf_proxy(proxies[proxy], ids[:n], i[:n], o[:n])
        assert got[0].shape == (n, 3) and got[1].shape == (n,)
        cases.assert_same(f"set <- {proxy}, n = {n}", got, [a[:n] for a in want])
    # the selection is not the result of any single material
    for fr, pdf in cases.per_material(proxy):
        assert not cases.same_bits(fr, want[0]).all() and not cases.same_bits(pdf, want[1]).all()


@pytest.mark.parametrize("proxy", KINDS)
def test_strided_and_soa_views(mset, proxies, proxy):
    ids, _ = cases.material_ids()
    i, o = cases.inputs()
    n = 4001
    want = [a[:n] for a in cases.expected(proxy)]
    cases.assert_same("aos", mset.evalp_pdf_proxy(proxies[proxy], ids[:n], i[:n], o[:n]), want)            # [n, 3]: stride 3
    fr, pdf = mset.evalp_pdf_proxy(proxies[proxy], ids[:n], np.ascontiguousarray(i[:n].T), np.ascontiguousarray(o[:n].T))
    assert fr.shape == (3, n)
    cases.assert_same("soa", (fr.T, pdf), want)                                                            # [3, n]: stride 1


def test_a_one_member_set_equals_the_single_material_values(cpu, proxies, oracle):
    i, o = cases.inputs()
    n = 8001
    i, o = i[:n], o[:n]
    free = ~cases.guarded(i, o)
    assert free.sum() > n // 2
    ids = np.zeros(n, np.int32)
    for m in (1, 2):
        s = djb.merl_set.from_tables([cases.tables()[m]], [cases.product_params()[m]], ctx=cpu)
        try:
            for kind in KINDS:
                fr, pdf = s.evalp_pdf_proxy(proxies[kind], ids, i, o)
                with np.errstate(all="ignore"):
                    wfr = np.asarray(oracle.eval(cases.oracle_materials()[m], i, o, None, "evalp"), np.float32)
                    wpdf = np.asarray(oracle.eval(oracle.microfacet(kind), i, o, cases.ORACLE_PARAMS[m], "pdf"), np.float32).reshape(-1)
                assert cases.same_bits(fr[free], wfr[free]).all() and cases.same_bits(pdf[free], wpdf[free]).all(), (m, kind)
                assert not fr[~free].view(np.uint32).any() and not pdf[~free].view(np.uint32).any()
        finally:
            s.close()


def test_facade_class_equals_the_python_mirror(cpu, proxies, tmp_path):
    src = os.path.join(ROOT, "tests", "api", "merl_set_light_facade.cpp")
    exe = tmp_path / "merl_set_light_facade"
    r = subprocess.run(["g++", "-O1", "-std=c++14", "-DNVERBOSE", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), src, "-L" + LIBDIR, "-ldjb_hip",
                        "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    paths = []
    for k in (0, 1):
        paths.append(str(tmp_path / f"m{k}.binary"))
        synth.write_merl_binary(paths[-1], cases.tables()[k])
    out = subprocess.run([str(exe)] + paths, env=dict(os.environ, DJB_DEVICE="cpu", DJB_QUIET="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = {}
    for line in out.stdout.splitlines():
        tag, *vals = line.split()
        rows.setdefault(tag, []).append([float.fromhex(v) for v in vals])
    ids = np.int32([0, 1, -1, 1, 0])
    o = np.float32([[0.1, 0.3, 0.9486833], [0.3, 0.2, 0.9327379], [0.5, 0.1, 0.8602325], [0.7, 0.0, 0.7141428], [0.9, -0.1, -0.4242641]])
    i = np.float32([[-0.1, -0.25, 0.9630680], [-0.3, -0.2, -0.9327379], [0.1, 0.5, 0.8602325], [-0.6, 0.1, 0.7937254], [0.2, 0.2, 0.9591663]])
    s = djb.merl_set.from_tables(cases.tables()[:2], cases.product_params()[:2], ctx=cpu)
    try:
        for kind in KINDS:
            fr, pdf = s.evalp_pdf_proxy(proxies[kind], ids, i, o)
            assert np.abs(fr[[0, 3]]).sum() > 0 and (pdf[[0, 3]] > 0).all()
            assert not fr[[1, 2, 4]].view(np.uint32).any() and not pdf[[1, 2, 4]].view(np.uint32).any()     # i.z < 0, inactive, o.z < 0
            assert cases.same_bits(np.float32(rows[kind]), np.concatenate([fr, pdf[:, None]], 1)).all(), (kind, rows[kind], fr, pdf)
    finally:
        s.close()


# ------------------------------------------------------------------ the C ABI's error cases
def _call(ctx, s, proxy, n=4, material=True, pdf=True, fr=True):
    lib = _lib.load()
    d = np.tile(np.float32([[0.3, 0.1, 0.9]]), (max(n, 1), 1)); ids = np.zeros(max(n, 1), np.int32)
    out, opdf = np.full((max(n, 1), 3), 7, np.float32), np.full(max(n, 1), 7, np.float32)
    vd, vout = djb._Vec(d), djb._Vec(out)
    st = lib.djb_merl_set_evalp_pdf_proxy_batch(ctx._h, s._h, proxy._h if proxy is not None else None, C.c_int64(n),
                                                C.c_void_p(ids.ctypes.data) if material else None, C.byref(vd.view), C.byref(vd.view),
                                                C.byref(vout.view) if fr else None, C.c_void_p(opdf.ctypes.data) if pdf else None, C.c_int(_lib.MEM_HOST))
    return st, lib.djb_last_error().decode(errors="replace"), out, opdf


def test_error_cases(cpu, mset, proxies):
    members = cases.product_members(cpu)[:1]
    bare = djb.merl_set(members, ctx=cpu)
    other = djb.Context("cpu")
    try:
        st, msg, out, opdf = _call(cpu, bare, proxies["ggx"])
        assert st == INVALID and "no proxy parameters" in msg, (st, msg)
        assert (out == 7).all() and (opdf == 7).all()
        for p in (djb.tabular(members[0], 16, True, ctx=cpu), djb.lambert(ctx=cpu)):
            st, msg, *_ = _call(cpu, mset, p)
            assert st == NOT_IMPLEMENTED and "ggx or beckmann" in msg, (st, msg)
        st, msg, *_ = _call(cpu, mset, None)
        assert st == INVALID and "proxy" in msg, (st, msg)
        st, msg, out, _ = _call(cpu, mset, proxies["ggx"], pdf=False)
        assert st == INVALID and "out_pdf" in msg and (out == 7).all(), (st, msg)
        st, msg, *_ = _call(cpu, mset, proxies["ggx"], fr=False)
        assert st == INVALID, (st, msg)
        assert "null output" in msg and "vec3 view" not in msg, msg      # a missing out_fr: this entry's own wording, not the eval entries'
        st, msg, *_ = _call(cpu, mset, proxies["ggx"], material=False)
        assert st == INVALID and "null material" in msg, (st, msg)
        st, msg, *_ = _call(cpu, mset, djb.ggx(ctx=other))
        assert st == INVALID and "different contexts" in msg, (st, msg)
        st, msg, *_ = _call(other, mset, djb.ggx(ctx=other))
        assert st == INVALID and "another context" in msg, (st, msg)
        st, msg, out, opdf = _call(cpu, mset, proxies["beckmann"], n=0)
        assert st == OK and (out == 7).all() and (opdf == 7).all(), (st, msg)
        for kind in KINDS:
            st, msg, out, opdf = _call(cpu, mset, proxies[kind])
            assert st == OK and (opdf > 0).all() and (out > 0).all(), (st, msg, out, opdf)
    finally:
        bare.close()
