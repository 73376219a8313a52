"""UTIA material sets on the host path (CPU context): djb.utia_set / djb_utia_set_* against the oracle's per-material results selected
by id (tests/utia_set_cases.py), the lifetime rules of the set, the error cases of the C ABI and the djb:: facade class.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import utia_set_cases as cases
from dj_brdf_amd import _lib, djb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dj_brdf_amd", "lib")
SIZES = (1, 2, 97)
INVALID = 1


@pytest.fixture(scope="module")
def cpu():
    return djb.cpu_context()


@pytest.fixture(scope="module")
def uset(cpu):
    """the three-material set; its sources are destroyed before the first call"""
    members = cases.product_members(cpu)
    s = djb.utia_set(members, ctx=cpu)
    for b in members:
        b.close()
    assert s.n_materials == cases.M
    yield s
    s.close()


def test_ids_cover_every_material_and_the_inactive_class():
    ids, bulk = cases.material_ids()
    cases.assert_ids_cover_every_class(ids, bulk)
    gids, gi, go = cases.grid_block()
    assert len(gids) == cases.GRID_N and not cases.active(gids[2::3], cases.M).any() and cases.active(gids[0::3], cases.M).all()


@pytest.mark.parametrize("want_cos", [0, 1])
def test_eval_equals_the_oracle_selection(uset, want_cos):
    ids, _ = cases.material_ids()
    i, o = cases.eval_inputs()
    op = "evalp" if want_cos else "eval"
    want = cases.expected_eval(op)
    mask = cases.compared(ids, i, o)
    call = uset.evalp if want_cos else uset.eval
    for n in (cases.N,) + SIZES:
        cases.assert_eval(f"{op}, n = {n}", call(ids[:n], i[:n], o[:n]), want[:n], mask[:n])
    act = cases.active(ids, cases.M)
    assert np.abs(np.nan_to_num(want[act])).sum() > 0 and not want[~act].view(np.uint32).any()
    # the three materials differ where it matters: the selection is not the result of any single one
    for per in cases.eval_per_material(op):
        assert not (cases.same_bits(per, want) | ~mask[:, None]).all()


@pytest.mark.parametrize("want_cos", [0, 1])
def test_grid_line_block(uset, want_cos):
    ids, i, o = cases.grid_block()
    op = "evalp" if want_cos else "eval"
    want = cases.grid_expected(op)
    got = (uset.evalp if want_cos else uset.eval)(ids, i, o)
    cases.assert_eval("grid lines, " + op, got, want, np.ones(len(ids), bool))
    assert np.abs(want).sum() > 0 and not got[2::3].view(np.uint32).any()


def test_the_set_outlives_its_context_and_repeats_handles():
    ctx = djb.Context("cpu")
    members = cases.product_members(ctx)
    layout = (0, 1, 0, 2, 1)
    s = djb.utia_set([members[k] for k in layout], ctx=ctx)
    for b in members:
        b.close()
    assert s.n_materials == len(layout)
    i, o = cases.eval_inputs()
    n = 4001
    ids = np.random.default_rng(3).integers(-1, len(layout) + 1, n).astype(np.int32)
    per = cases.eval_per_material("evalp")
    want = np.zeros((n, 3), np.float32)
    for e, k in enumerate(layout):
        want[ids == e] = per[k][:n][ids == e]
    mask = cases.defined(i[:n], o[:n]) | ~cases.active(ids, len(layout))
    cases.assert_eval("repeated handles", s.evalp(ids, i[:n], o[:n]), want, mask)
    ctx.close()
    s.close()                                        # after its context


def test_from_tables(cpu):
    ids, i, o = cases.grid_block()
    s = djb.utia_set.from_tables(cases.tables()[:2], ctx=cpu)
    try:
        assert s.n_materials == 2
        two = np.where(ids == 2, -1, ids).astype(np.int32)
        want = np.where((two >= 0)[:, None], cases.grid_expected("eval"), np.float32(0))
        cases.assert_eval("from_tables", s.eval(two, i, o), want, np.ones(len(ids), bool))
    finally:
        s.close()


def test_facade_class_equals_the_members_own_eval(tmp_path):
    src = os.path.join(ROOT, "tests", "api", "utia_set_facade.cpp")
    exe = tmp_path / "utia_set_facade"
    r = subprocess.run(["g++", "-O1", "-std=c++14", "-DNVERBOSE", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), src, "-L" + LIBDIR, "-ldjb_hip",
                        "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], env=dict(os.environ, DJB_DEVICE="cpu", DJB_QUIET="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hits checked" in out.stdout and "0 differ" in out.stdout, out.stdout


# ------------------------------------------------------------------ the C ABI's error cases
def _create(ctx, handles, n=None):
    lib = _lib.load()
    n = len(handles) if n is None else n
    ptrs = (C.c_void_p * max(len(handles), 1))(*handles)
    out = C.c_void_p()
    st = lib.djb_utia_set_create(ctx._h, C.c_int(n), ptrs, C.byref(out))
    msg = lib.djb_last_error().decode(errors="replace")
    if st == 0:
        lib.djb_utia_set_destroy(out)
    return st, msg


def _eval(ctx, s, material=True, output=True, n=4):
    lib = _lib.load()
    d = np.tile(np.float32([[0.3, 0.1, 0.9]]), (n, 1)); ids = np.zeros(n, np.int32); out = np.zeros((n, 3), np.float32)
    vd, vout = djb._Vec(d), djb._Vec(out)
    st = lib.djb_utia_set_eval_batch(ctx._h, s._h, C.c_int64(n), C.c_void_p(ids.ctypes.data) if material else None, C.byref(vd.view), C.byref(vd.view),
                                     C.c_int(1), C.byref(vout.view) if output else None, C.c_int(_lib.MEM_HOST))
    return st, lib.djb_last_error().decode(errors="replace")


def test_error_cases(cpu, uset):
    members = cases.product_members(cpu)[:1]
    h = members[0]._h.value
    st, msg = _create(cpu, [], n=0)
    assert st == INVALID and "1 .. 256" in msg, (st, msg)
    st, msg = _create(cpu, [h] * 257)
    assert st == INVALID and "1 .. 256" in msg, (st, msg)
    st, msg = _create(cpu, [h] * 2)
    assert st == 0, msg
    ggx = djb.ggx(ctx=cpu)
    st, msg = _create(cpu, [h, ggx._h.value])
    assert st == INVALID and "member 1" in msg and "not a utia" in msg, (st, msg)
    st, msg = _create(cpu, [h, None])
    assert st == INVALID and "member 1" in msg and "null" in msg, (st, msg)
    other = djb.Context("cpu")
    foreign = djb.utia.from_table(cases.tables()[1], ctx=other)
    st, msg = _create(cpu, [h, foreign._h.value])
    assert st == INVALID and "member 1" in msg and "another context" in msg, (st, msg)
    st, msg = _eval(cpu, uset, output=False)
    assert st == INVALID and "null output" in msg, (st, msg)
    st, msg = _eval(cpu, uset, material=False)
    assert st == INVALID and "null material" in msg, (st, msg)
    st, msg = _eval(other, uset)
    assert st == INVALID and "another context" in msg, (st, msg)
    st, msg = _eval(cpu, uset)
    assert st == 0, msg
