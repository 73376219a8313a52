"""SGD / ABC model sets on the host path (CPU context): djb.model_set / djb_model_set_* against the oracle's per-material results selected
by id (tests/model_set_cases.py) -- the main set, the wall block and the 100 published rows, both kinds, eval and evalp --, the three
constructors, the lifetime rules of the set, the error cases of the C ABI and the djb:: facade class.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import model_set_cases as cases
from dj_brdf_amd import _lib, djb, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dj_brdf_amd", "lib")
SIZES = (1, 2, 97)
INVALID = 1
OPS = ((0, "eval"), (1, "evalp"))


@pytest.fixture(scope="module")
def cpu():
    return djb.cpu_context()


def _members(kind, ctx, rows=None):
    cls = djb.sgd if kind == "sgd" else djb.abc
    return [cls.from_params(r, ctx=ctx) for r in (cases.rows(kind) if rows is None else rows)]


@pytest.fixture(scope="module")
def sets(cpu):
    """the main set of each kind, built from brdf objects that are closed before the first call"""
    out = {}
    for kind in cases.KINDS:
        members = _members(kind, cpu)
        out[kind] = djb.model_set(members, ctx=cpu)
        for b in members:
            b.close()
        assert out[kind].n_materials == cases.M and out[kind].kind == kind
    yield out
    for s in out.values():
        s.close()


def test_inputs_are_what_the_cases_say():
    ids, bulk = cases.material_ids()
    cases.assert_ids_cover_every_class(ids, bulk, cases.M)
    cases.assert_rows_mix_the_tiers()
    cases.assert_wall_block_is_at_the_wall()


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("want_cos,op", OPS)
def test_eval_equals_the_oracle_selection(sets, kind, want_cos, op):
    s = sets[kind]
    ids, _ = cases.material_ids()
    i, o = cases.eval_inputs()
    want = cases.expected_eval(kind, op)
    call = s.evalp if want_cos else s.eval
    for n in (cases.N,) + SIZES:
        cases.assert_eval(f"{kind} {op}, n = {n}", call(ids[:n], i[:n], o[:n]), want[:n])
    act = cases.active(ids, cases.M)
    assert np.abs(np.nan_to_num(want[act], posinf=0, neginf=0)).sum() > 0 and not want[~act].view(np.uint32).any()
    # the rows differ where it matters: the selection is not the result of any single one
    for per in cases.eval_per_material(kind, op):
        assert not cases.same_bits(per, want).all()


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("want_cos,op", OPS)
def test_wall_block(sets, kind, want_cos, op):
    ids, i, o = cases.wall_block(kind)
    want = cases.wall_expected(kind, op)
    got = (sets[kind].evalp if want_cos else sets[kind].eval)(ids, i, o)
    cases.assert_eval(f"wall block, {kind} {op}", got, want)
    assert np.abs(want).sum() > 0 and not np.asarray(got)[2::3].view(np.uint32).any()
    for per in cases.wall_per_material(kind, op):
        assert not cases.same_bits(per, want).all()


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("want_cos,op", OPS)
def test_the_hundred_published_rows(cpu, kind, want_cos, op):
    s = djb.model_set.from_names(kind, synth.MERL_NAMES, ctx=cpu)
    try:
        assert s.n_materials == cases.PUBLISHED_M == 100 and s.kind == kind
        i, o = cases.eval_inputs()
        got = (s.evalp if want_cos else s.eval)(cases.published_ids(), i, o)
        cases.assert_eval(f"published rows, {kind} {op}", got, cases.published_expected(kind, op))
    finally:
        s.close()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_the_three_constructors_give_the_same_bits(cpu, sets, kind):
    ids, i, o = cases.wall_block(kind)
    ref = np.asarray(sets[kind].evalp(ids, i, o))
    by_rows = djb.model_set.from_rows(kind, cases.rows(kind), ctx=cpu)
    names = list(cases.PUBLISHED)
    by_names = djb.model_set.from_names(kind, names, ctx=cpu)
    try:
        assert cases.same_bits(np.asarray(by_rows.evalp(ids, i, o)), ref).all()
        low = np.where(cases.active(ids, len(names)), ids, -1).astype(np.int32)      # the published rows are rows 0 .. 2 of the main set
        want = np.where((low >= 0)[:, None], ref, np.float32(0))
        assert by_names.n_materials == len(names) and cases.same_bits(np.asarray(by_names.evalp(low, i, o)), want).all()
    finally:
        by_rows.close(); by_names.close()
    if kind == "sgd":                                    # an sgd row also answers to its alias
        from dj_brdf_amd import param_tables
        import csv
        with open(os.path.join(ROOT, "dj_brdf_amd", "data", "sgd_params.csv")) as f:
            alias = next(r for r in csv.DictReader(f) if r["other_name"] and r["other_name"] != r["name"])
        a = djb.model_set.from_names("sgd", [alias["other_name"]], ctx=cpu)
        b = djb.model_set.from_rows("sgd", [param_tables.sgd_params(alias["name"])], ctx=cpu)
        zero = np.zeros(len(ids), np.int32)
        assert cases.same_bits(np.asarray(a.eval(zero, i, o)), np.asarray(b.eval(zero, i, o))).all()
        a.close(); b.close()
    with pytest.raises(djb.exc) as e:
        djb.model_set.from_names(kind, ["gold-metallic-paint", "no-such-material"], ctx=cpu)
    with pytest.raises(djb.exc) as single:
        (djb.sgd if kind == "sgd" else djb.abc)("no-such-material", ctx=cpu)
    assert e.value.status == single.value.status == 8 and str(e.value) == str(single.value), (str(e.value), str(single.value))


def test_the_set_outlives_its_context_and_repeats_handles():
    ctx = djb.Context("cpu")
    members = _members("sgd", ctx)
    layout = (0, 4, 0, 2, 5)
    s = djb.model_set([members[k] for k in layout], ctx=ctx)
    for b in members:
        b.close()
    assert s.n_materials == len(layout)
    i, o = cases.eval_inputs()
    n = 4001
    ids = np.random.default_rng(3).integers(-1, len(layout) + 1, n).astype(np.int32)
    per = cases.eval_per_material("sgd", "evalp")
    want = np.zeros((n, 3), np.float32)
    for e, k in enumerate(layout):
        want[ids == e] = per[k][:n][ids == e]
    cases.assert_eval("repeated handles", s.evalp(ids, i[:n], o[:n]), want)
    ctx.close()
    s.close()                                        # after its context


def test_facade_class_equals_the_members_own_eval(tmp_path):
    src = os.path.join(ROOT, "tests", "api", "model_set_facade.cpp")
    exe = tmp_path / "model_set_facade"
    r = subprocess.run(["g++", "-O1", "-std=c++14", "-DNVERBOSE", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), src, "-L" + LIBDIR, "-ldjb_hip",
                        "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], env=dict(os.environ, DJB_DEVICE="cpu", DJB_QUIET="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hits checked" in out.stdout and " 0 differ" in out.stdout, out.stdout


def test_the_gpu_entry_fails_loudly_without_a_gpu():
    """a GPU context is never answered by the host path: without a device it cannot be had at all"""
    if djb.device_count() > 0:                       # tests/test_gpu_model_set.py covers the GPU entry
        return
    with pytest.raises((djb.exc, ImportError, RuntimeError)) as e:
        djb.model_set.from_rows("abc", cases.rows("abc"), ctx=djb.Context(0))
    assert getattr(e.value, "status", 7) in (6, 7), str(e.value)                    # DJB_ERR_HIP / DJB_ERR_NO_DEVICE


# ------------------------------------------------------------------ the C ABI's error cases
def _create_rows(ctx, kind, n, rows=True, out=True):
    lib = _lib.load()
    r = np.ascontiguousarray(np.tile(cases.rows("sgd" if kind == 6 else "abc")[:1], (max(n, 1), 1))) if rows else None
    h = C.c_void_p()
    st = lib.djb_model_set_create(ctx._h if ctx else None, C.c_int(kind), C.c_int(n), C.c_void_p(r.ctypes.data) if rows else None, C.byref(h) if out else None)
    msg = lib.djb_last_error().decode(errors="replace")
    if st == 0:
        lib.djb_model_set_destroy(h)
    return st, msg


def _create(ctx, handles, n=None):
    lib = _lib.load()
    n = len(handles) if n is None else n
    ptrs = (C.c_void_p * max(len(handles), 1))(*handles)
    out = C.c_void_p()
    st = lib.djb_model_set_create_from_brdfs(ctx._h, C.c_int(n), ptrs, C.byref(out))
    msg = lib.djb_last_error().decode(errors="replace")
    if st == 0:
        lib.djb_model_set_destroy(out)
    return st, msg


def _eval(ctx, s, material=True, output=True, n=4):
    lib = _lib.load()
    d = np.tile(np.float32([[0.3, 0.1, 0.9]]), (n, 1)); ids = np.zeros(n, np.int32); out = np.zeros((n, 3), np.float32)
    vd, vout = djb._Vec(d), djb._Vec(out)
    st = lib.djb_model_set_eval_batch(ctx._h if ctx else None, s._h if s else None, C.c_int64(n), C.c_void_p(ids.ctypes.data) if material else None,
                                      C.byref(vd.view), C.byref(vd.view), C.c_int(1), C.byref(vout.view) if output else None, C.c_int(_lib.MEM_HOST))
    return st, lib.djb_last_error().decode(errors="replace")


def test_error_cases(cpu, sets):
    SGD, ABC = 6, 7
    for kw in (dict(rows=False), dict(out=False)):
        st, msg = _create_rows(cpu, SGD, 2, **kw)
        assert st == INVALID and "null argument" in msg, (st, msg)
    st, msg = _create_rows(None, SGD, 2)
    assert st == INVALID and "null argument" in msg, (st, msg)
    st, msg = _create_rows(cpu, SGD, 0)
    assert st == INVALID and "1 .. 65536" in msg, (st, msg)
    st, msg = _create_rows(cpu, ABC, cases.MODEL_SET_MAX + 1)
    assert st == INVALID and "1 .. 65536" in msg, (st, msg)
    st, msg = _create_rows(cpu, ABC, cases.MODEL_SET_MAX)
    assert st == 0, msg
    st, msg = _create_rows(cpu, 3, 2)                                     # DJB_KIND_MERL
    assert st == INVALID and "sgd" in msg and "abc" in msg, (st, msg)
    a, b = _members("sgd", cpu)[0], _members("abc", cpu)[0]
    h = a._h.value
    st, msg = _create(cpu, [], n=0)
    assert st == INVALID and "1 .. 65536" in msg, (st, msg)
    st, msg = _create(cpu, [h] * 2)
    assert st == 0, msg
    st, msg = _create(cpu, [h, b._h.value])
    assert st == INVALID and "member 1" in msg and "one kind" in msg, (st, msg)
    merl = djb.merl.from_table(synth.merl_table(), ctx=cpu)
    st, msg = _create(cpu, [h, merl._h.value])
    assert st == INVALID and "member 1" in msg and "not an sgd or abc" in msg, (st, msg)
    st, msg = _create(cpu, [h, None])
    assert st == INVALID and "member 1" in msg and "null" in msg, (st, msg)
    other = djb.Context("cpu")
    foreign = djb.sgd.from_params(cases.rows("sgd")[1], ctx=other)
    st, msg = _create(cpu, [h, foreign._h.value])
    assert st == INVALID and "member 1" in msg and "another context" in msg, (st, msg)
    s = sets["sgd"]
    st, msg = _eval(cpu, None)
    assert st == INVALID and "null model set" in msg, (st, msg)
    st, msg = _eval(None, s)
    assert st == INVALID and "null ctx" in msg, (st, msg)
    st, msg = _eval(cpu, s, output=False)
    assert st == INVALID and "null output" in msg, (st, msg)
    st, msg = _eval(cpu, s, material=False)
    assert st == INVALID and "null material" in msg, (st, msg)
    st, msg = _eval(other, s)
    assert st == INVALID and "another context" in msg, (st, msg)
    st, msg = _eval(cpu, s)
    assert st == 0, msg
