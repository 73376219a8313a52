"""Microfacet sets on the host path (CPU context): djb.microfacet_set / djb_microfacet_set_* against the oracle's per-material results
selected by id (tests/microfacet_set_cases.py) -- every op on the main set and the mixing block, both kinds --, the uniform-Fresnel set
against the mixed one, the two constructors, set_params, the lifetime rules of the set, the error cases of the C ABI and the djb::
facade class.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import microfacet_set_cases as cases
from dj_brdf_amd import _lib, djb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dj_brdf_amd", "lib")
SIZES = (1, 2, 97)
INVALID, NOT_IMPLEMENTED = 1, 5
GGX, BECKMANN = 1, 0


@pytest.fixture(scope="module")
def cpu():
    return djb.cpu_context()


@pytest.fixture(scope="module")
def sets(cpu):
    """the main set of each kind, built from brdf objects that are closed before the first call"""
    out = {}
    for kind in cases.KINDS:
        members, params = cases.product_members(kind, cpu)
        out[kind] = djb.microfacet_set(members, params, ctx=cpu)
        for b in members:
            b.close()
        assert out[kind].n_materials == cases.M and out[kind].kind == kind
    yield out
    for s in out.values():
        s.close()


def check_ops(tag, s, ids, i, o, so, u1, u2, want_eval, want_sample):
    """every op of a set on one batch: want_eval = {op: array}, want_sample = (weight, i, pdf, i of sample)"""
    for op in cases.EVAL_OPS:
        cases.assert_bits(f"{tag} {op}", getattr(s, op)(ids, i, o), want_eval[op])
    for cos, op in ((False, "eval"), (True, "evalp")):
        fr, pdf = s.eval_pdf(ids, i, o, cos=cos)
        cases.assert_bits(f"{tag} fused {op}", fr, want_eval[op])
        cases.assert_bits(f"{tag} fused {op}: pdf", pdf, want_eval["pdf"])
    for name, g, w in zip(("weight", "i", "pdf"), s.evalp_is(ids, u1, u2, so), want_sample[:3]):
        cases.assert_bits(f"{tag} evalp_is {name}", g, w)
    cases.assert_bits(f"{tag} sample", s.sample(ids, u1, u2, so), want_sample[3])


def test_inputs_are_what_the_cases_say():
    ids, bulk = cases.material_ids()
    cases.assert_ids_cover_every_class(ids, bulk, cases.M)
    cases.assert_materials_are_what_the_module_says()
    cases.assert_mix_block_mixes()
    _, u1, u2 = cases.sample_inputs()
    for u in (u1, u2):
        assert (u == 0).any() and (u == 1).any() and (u < 0).any() and (u > 1).any()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_every_op_equals_the_oracle_selection(sets, kind):
    s = sets[kind]
    ids, _ = cases.material_ids()
    i, o = cases.eval_inputs()
    so, u1, u2 = cases.sample_inputs()
    want_eval = {op: cases.expected_eval(kind, op) for op in cases.EVAL_OPS}
    want_sample = cases.expected_sample(kind)
    for n in (cases.N,) + SIZES:
        check_ops(f"{kind}, n = {n}", s, ids[:n], i[:n], o[:n], so[:n], u1[:n], u2[:n], {k: v[:n] for k, v in want_eval.items()},
                  [w[:n] for w in want_sample])
    act = cases.active(ids, cases.M)
    for want in list(want_eval.values()) + list(want_sample):
        assert np.abs(np.nan_to_num(want[act], posinf=0, neginf=0)).sum() > 0 and not want[~act].view(np.uint32).any()
    # the materials differ where it matters: the selection is not the result of any single one
    for op in cases.EVAL_OPS:
        for per in cases.eval_per_material(kind, op):
            assert not cases.same_bits(per, want_eval[op]).all()
    for per in cases.sample_per_material(kind):
        assert not cases.same_bits(per[1], want_sample[1]).all()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_mixing_block(sets, kind):
    ids, i, o, u1, u2 = cases.mix_block()
    want = cases.mix_expected(kind)
    check_ops(f"mixing block, {kind}", sets[kind], ids, i, o, o, u1, u2, want, want["evalp_is"] + (want["sample"],))
    assert np.abs(want["evalp"]).sum() > 0 and not np.asarray(sets[kind].evalp(ids, i, o))[2::3].view(np.uint32).any()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_one_fresnel_kind_and_a_mixed_set_give_the_same_bits(cpu, kind):
    nu = len(cases.UNIFORM)
    uni, mixed = cases.product_set(kind, cpu, cases.UNIFORM), cases.product_set(kind, cpu, cases.MIXED)
    try:
        i, o = cases.eval_inputs()
        so, u1, u2 = cases.sample_inputs()
        ids_u, ids_m = cases.material_ids(nu)[0], cases.ids_below(len(cases.MIXED), nu)
        for s, ids, mats, limit in ((uni, ids_u, cases.UNIFORM, None), (mixed, ids_m, cases.MIXED, nu)):
            check_ops(f"{kind}, {len(mats)} materials", s, ids, i, o, so, u1, u2,
                      {op: cases.expected_eval(kind, op, mats, limit) for op in cases.EVAL_OPS}, cases.expected_sample(kind, mats, limit))
        # ... and on the SAME ids each other's
        for op in ("evalp", "pdf"):
            assert cases.same_bits(np.asarray(getattr(uni, op)(ids_m, i, o)), np.asarray(getattr(mixed, op)(ids_m, i, o))).all()
        for a, b in zip(uni.evalp_is(ids_m, u1, u2, so), mixed.evalp_is(ids_m, u1, u2, so)):
            assert cases.same_bits(np.asarray(a), np.asarray(b)).all()
    finally:
        uni.close(); mixed.close()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_the_two_constructors_give_the_same_bits(cpu, sets, kind):
    ids, i, o, u1, u2 = cases.mix_block()
    plain = cases.product_set(kind, cpu)
    try:
        assert plain.kind == kind and plain.n_materials == cases.M
        for op in cases.EVAL_OPS:
            assert cases.same_bits(np.asarray(getattr(plain, op)(ids, i, o)), np.asarray(getattr(sets[kind], op)(ids, i, o))).all()
        for a, b in zip(plain.evalp_is(ids, u1, u2, o), sets[kind].evalp_is(ids, u1, u2, o)):
            assert cases.same_bits(np.asarray(a), np.asarray(b)).all()
    finally:
        plain.close()
    # params = None: params::standard() for every member
    members, _ = cases.product_members(kind, cpu)
    std = djb.microfacet_set(members, ctx=cpu)
    same = cases.product_set(kind, cpu, tuple((f, sh, None) for f, sh, _ in cases.MATERIALS))
    assert cases.same_bits(np.asarray(std.evalp(ids, i, o)), np.asarray(same.evalp(ids, i, o))).all()
    std.close(); same.close()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_set_params_is_seen_by_the_next_call(cpu, kind):
    ids, i, o, u1, u2 = cases.mix_block()
    rolled = cases.MATERIALS[1:] + cases.MATERIALS[:1]
    moved = tuple((m[0], m[1], r[2]) for m, r in zip(cases.MATERIALS, rolled))          # every material with its neighbour's params
    s, want = cases.product_set(kind, cpu), cases.product_set(kind, cpu, moved)
    try:
        before = np.asarray(s.evalp(ids, i, o)).copy()
        s.set_params([cases.mk_params(m[2]) for m in moved])
        after = np.asarray(s.evalp(ids, i, o))
        import oraclelib
        O = oraclelib.oracle()
        per = [O.eval(om, i, o, m[2], "evalp") for om, m in zip(cases.oracle_materials(kind), moved)]
        cases.assert_bits(f"{kind} after set_params", after, cases.select(per, ids, cases.M))
        assert not cases.same_bits(before, after).all()
        assert cases.same_bits(after, np.asarray(want.evalp(ids, i, o))).all()
        with pytest.raises(djb.exc):
            s.set_params([cases.mk_params(None)] * (cases.M - 1))
    finally:
        s.close(); want.close()


def test_the_set_outlives_its_context_and_repeats_handles():
    ctx = djb.Context("cpu")
    members, params = cases.product_members("ggx", ctx)
    layout = (0, 4, 0, 2, 5)
    s = djb.microfacet_set([members[k] for k in layout], [params[k] for k in layout], ctx=ctx)
    members[4].set_shadow(True)                          # the set copied: a later change of a member is not seen
    for b in members:
        b.close()
    assert s.n_materials == len(layout)
    i, o = cases.eval_inputs()
    n = 4001
    ids = np.random.default_rng(3).integers(-1, len(layout) + 1, n).astype(np.int32)
    per = cases.eval_per_material("ggx", "evalp")
    want = np.zeros((n, 3), np.float32)
    for e, k in enumerate(layout):
        want[ids == e] = per[k][:n][ids == e]
    cases.assert_bits("repeated handles", s.evalp(ids, i[:n], o[:n]), want)
    ctx.close()
    s.close()                                        # after its context


def test_facade_class_equals_the_members_own_calls(tmp_path):
    src = os.path.join(ROOT, "tests", "api", "microfacet_set_facade.cpp")
    exe = tmp_path / "microfacet_set_facade"
    r = subprocess.run(["g++", "-O1", "-std=c++14", "-DNVERBOSE", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), src, "-L" + LIBDIR, "-ldjb_hip",
                        "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], env=dict(os.environ, DJB_DEVICE="cpu", DJB_QUIET="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hits checked" in out.stdout and " 0 differ" in out.stdout, out.stdout


def test_the_gpu_entry_fails_loudly_without_a_gpu():
    """a GPU context is never answered by the host path: without a device it cannot be had at all"""
    if djb.device_count() > 0:                       # tests/test_gpu_microfacet_set.py covers the GPU entry
        return
    with pytest.raises((djb.exc, ImportError, RuntimeError)) as e:
        cases.product_set("ggx", djb.Context(0))
    assert getattr(e.value, "status", 7) in (6, 7), str(e.value)                    # DJB_ERR_HIP / DJB_ERR_NO_DEVICE


# ------------------------------------------------------------------ the C ABI's error cases
def _materials(n, fresnel_kind=0, params_kind=0):
    arr = (_lib.MicrofacetMaterial * max(n, 1))()
    for m in range(n):
        arr[m].fresnel.kind, arr[m].shadow, arr[m].params.kind = fresnel_kind, 1, params_kind
    return arr


def _create(ctx, kind, n, arr=True, out=True, **kw):
    lib = _lib.load()
    mats = _materials(n, **kw) if arr else None
    h = C.c_void_p()
    st = lib.djb_microfacet_set_create(ctx._h if ctx else None, C.c_int(kind), C.c_int(n), mats, C.byref(h) if out else None)
    msg = lib.djb_last_error().decode(errors="replace")
    if st == 0:
        lib.djb_microfacet_set_destroy(h)
    return st, msg


def _from_brdfs(ctx, handles, n=None, params=None):
    lib = _lib.load()
    n = len(handles) if n is None else n
    ptrs = (C.c_void_p * max(len(handles), 1))(*handles)
    out = C.c_void_p()
    st = lib.djb_microfacet_set_create_from_brdfs(ctx._h, C.c_int(n), ptrs, params, C.byref(out))
    msg = lib.djb_last_error().decode(errors="replace")
    if st == 0:
        lib.djb_microfacet_set_destroy(out)
    return st, msg


def _eval(ctx, s, want=6, material=True, fr=True, pdf=True, i=True, n=4):
    lib = _lib.load()
    d = np.tile(np.float32([[0.3, 0.1, 0.9]]), (n, 1)); ids = np.zeros(n, np.int32); out = np.zeros((n, 3), np.float32); p = np.zeros(n, np.float32)
    vd, vout = djb._Vec(d), djb._Vec(out)
    st = lib.djb_microfacet_set_eval_batch(ctx._h if ctx else None, s._h if s else None, C.c_int64(n), C.c_void_p(ids.ctypes.data) if material else None,
                                           C.byref(vd.view) if i else None, C.byref(vd.view), C.c_int(want), C.byref(vout.view) if fr else None,
                                           C.c_void_p(p.ctypes.data) if pdf else None, C.c_int(_lib.MEM_HOST))
    return st, lib.djb_last_error().decode(errors="replace")


def _sample(ctx, s, w=True, i=True, pdf=True, u=True, n=4):
    lib = _lib.load()
    d = np.tile(np.float32([[0.3, 0.1, 0.9]]), (n, 1)); ids = np.zeros(n, np.int32); uu = np.full(n, 0.5, np.float32)
    ow, oi, p = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    vd, vw, vi = djb._Vec(d), djb._Vec(ow), djb._Vec(oi)
    st = lib.djb_microfacet_set_sample_batch(ctx._h, s._h, C.c_int64(n), C.c_void_p(ids.ctypes.data), C.c_void_p(uu.ctypes.data) if u else None,
                                             C.c_void_p(uu.ctypes.data), C.byref(vd.view), C.byref(vw.view) if w else None, C.byref(vi.view) if i else None,
                                             C.c_void_p(p.ctypes.data) if pdf else None, C.c_int(_lib.MEM_HOST))
    return st, lib.djb_last_error().decode(errors="replace")


def test_error_cases(cpu, sets):
    for kw in (dict(arr=False), dict(out=False)):
        st, msg = _create(cpu, GGX, 2, **kw)
        assert st == INVALID and "null argument" in msg, (st, msg)
    st, msg = _create(None, GGX, 2)
    assert st == INVALID and "null argument" in msg, (st, msg)
    st, msg = _create(cpu, GGX, 0)                                         # M = 0 and M = MAX + 1
    assert st == INVALID and "1 .. 65536" in msg, (st, msg)
    st, msg = _create(cpu, BECKMANN, cases.SET_MAX + 1)
    assert st == INVALID and "1 .. 65536" in msg, (st, msg)
    st, msg = _create(cpu, BECKMANN, cases.SET_MAX)
    assert st == 0, msg
    st, msg = _create(cpu, 2, 2)                                           # DJB_KIND_TABULAR
    assert st == INVALID and "ggx" in msg and "beckmann" in msg, (st, msg)
    st, msg = _create(cpu, GGX, 3, fresnel_kind=4)                         # a spline row
    assert st == NOT_IMPLEMENTED and "spline" in msg and "material 0" in msg, (st, msg)
    st, msg = _create(cpu, GGX, 3, fresnel_kind=5)                         # DJB_FRESNEL_HOST
    assert st == INVALID and "material 0" in msg, (st, msg)
    st, msg = _create(cpu, GGX, 3, params_kind=0x100 | 1)                  # a flagged djb_params
    assert st == INVALID and "DJB_PARAMS_RESOLVED_FOLLOWS" in msg, (st, msg)
    st, msg = _create(cpu, GGX, 3, params_kind=3)                          # lambert::params
    assert st == INVALID, (st, msg)
    g, b = djb.ggx(ctx=cpu), djb.beckmann(ctx=cpu)
    h = g._h.value
    st, msg = _from_brdfs(cpu, [], n=0)
    assert st == INVALID and "1 .. 65536" in msg, (st, msg)
    st, msg = _from_brdfs(cpu, [h] * 2)
    assert st == 0, msg
    st, msg = _from_brdfs(cpu, [h, h, b._h.value, h])                      # mixed kinds: the first odd member is named
    assert st == INVALID and "member 2" in msg and "one kind" in msg and "beckmann" in msg, (st, msg)
    lam = djb.lambert(ctx=cpu)
    st, msg = _from_brdfs(cpu, [h, lam._h.value])
    assert st == INVALID and "member 1" in msg and "not a ggx or beckmann" in msg, (st, msg)
    spl = djb.ggx(cases.mk_fresnel(cases.golden_cases._SPLINE), True, ctx=cpu)         # a spline member
    st, msg = _from_brdfs(cpu, [h, spl._h.value])
    assert st == NOT_IMPLEMENTED and "material 1" in msg and "spline" in msg, (st, msg)
    st, msg = _from_brdfs(cpu, [h, None])
    assert st == INVALID and "member 1" in msg and "null" in msg, (st, msg)
    flagged = (_lib.Params * 2)(); flagged[1].kind = 0x100
    st, msg = _from_brdfs(cpu, [h, h], params=flagged)
    assert st == INVALID and "[1]" in msg and "DJB_PARAMS_RESOLVED_FOLLOWS" in msg, (st, msg)
    other = djb.Context("cpu")
    foreign = djb.ggx(ctx=other)
    st, msg = _from_brdfs(cpu, [h, foreign._h.value])
    assert st == INVALID and "member 1" in msg and "another context" in msg, (st, msg)
    s = sets["ggx"]
    st, msg = _eval(cpu, None)
    assert st == INVALID and "null microfacet set" in msg, (st, msg)
    st, msg = _eval(None, s)
    assert st == INVALID and "null ctx" in msg, (st, msg)
    for want, kw in ((6, dict(fr=False)), (6, dict(pdf=False)), (1, dict(fr=False)), (4, dict(pdf=False)), (5, dict(i=False))):       # a missing array
        st, msg = _eval(cpu, s, want, **kw)
        assert st == INVALID and "null" in msg, (want, kw, st, msg)
    for want, kw in ((4, dict(fr=False)), (1, dict(pdf=False)), (2, dict(pdf=False))):     # not asked for: may be NULL
        st, msg = _eval(cpu, s, want, **kw)
        assert st == 0, (want, kw, msg)
    for want in (0, 3, 7, 8):
        st, msg = _eval(cpu, s, want)
        assert st == INVALID and "want" in msg, (want, st, msg)
    st, msg = _eval(cpu, s, material=False)
    assert st == INVALID and "null material" in msg, (st, msg)
    st, msg = _eval(other, s)                                              # a set of another context
    assert st == INVALID and "another context" in msg, (st, msg)
    st, msg = _eval(cpu, s)
    assert st == 0, msg
    for kw in (dict(i=False), dict(w=False), dict(pdf=False), dict(u=False), dict(u=False, w=False, pdf=False)):
        st, msg = _sample(cpu, s, **kw)
        assert st == INVALID and "null" in msg, (kw, st, msg)
    for kw in ({}, dict(w=False, pdf=False)):                              # evalp_is, sample
        st, msg = _sample(cpu, s, **kw)
        assert st == 0, (kw, msg)
    lib = _lib.load()
    assert lib.djb_microfacet_set_set_params(s._h, None) == INVALID and lib.djb_microfacet_set_set_params(None, flagged) == INVALID
    assert lib.djb_microfacet_set_set_params(s._h, (_lib.Params * cases.M)(*([flagged[1]] * cases.M))) == INVALID
    assert lib.djb_microfacet_set_info(None, None, None) == INVALID and lib.djb_microfacet_set_destroy(None) == 0
