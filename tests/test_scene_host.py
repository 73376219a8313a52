"""Scenes on the host path (CPU context): djb.scene / djb_scene_* against the oracle's per-material results selected by scene id
(tests/scene_cases.py) -- the 18-slot scene, the permuted table with a slot without material and an alias, scenes with fewer member sets,
the refusals of the C ABI and djb_scene_info.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import merl_set_cases
import model_set_cases
import scene_cases as cases
import utia_set_cases
from dj_brdf_amd import _lib, djb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dj_brdf_amd", "lib")
INVALID = 1
OPS = ((0, "eval"), (1, "evalp"))
KIND_VALUE = {"merl": 3, "utia": 4, "sgd": 6, "abc": 7}


@pytest.fixture(scope="module")
def cpu():
    return djb.cpu_context()


@pytest.fixture(scope="module")
def members(cpu):
    """the four member sets, built as the set tests build them; their sources are closed before the first call"""
    out = {}
    src = merl_set_cases.product_members(cpu)
    out["merl"] = djb.merl_set(src, ctx=cpu)
    for b in src:
        b.close()
    src = utia_set_cases.product_members(cpu)
    out["utia"] = djb.utia_set(src, ctx=cpu)
    for b in src:
        b.close()
    for kind in model_set_cases.KINDS:
        out[kind] = djb.model_set.from_rows(kind, model_set_cases.rows(kind), ctx=cpu)
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(scope="module")
def main(cpu, members):
    s = djb.scene(slots=cases.TABLE, ctx=cpu, **members)
    yield s
    s.close()


def test_inputs_are_what_the_cases_say():
    cases.assert_inputs_are_what_the_module_says()


def test_info(main, members):
    assert main.n_slots == cases.N_SLOTS == 18
    assert main.members == (merl_set_cases.M, utia_set_cases.M, model_set_cases.M, model_set_cases.M) == (3, 3, 6, 6)
    s = djb.scene(utia=members["utia"], slots=[("utia", 2), None], ctx=main.ctx)
    assert s.n_slots == 2 and s.members == (0, 3, 0, 0)
    s.close()
    lib = _lib.load()
    assert lib.djb_scene_info(None, None, None) == INVALID and "null scene" in lib.djb_last_error().decode()
    assert lib.djb_scene_info(main._h, None, None) == 0 and lib.djb_scene_destroy(None) == 0


@pytest.mark.parametrize("want_cos,op", OPS)
def test_eval_equals_the_oracle_selection(main, want_cos, op):
    ids, _ = cases.material_ids()
    i, o = cases.eval_inputs()
    want = cases.expected(op)
    mask = cases.compared(ids, i, o)
    call = main.evalp if want_cos else main.eval
    for n in (cases.N, 1, 2, 97):
        cases.assert_eval(f"{op}, n = {n}", call(ids[:n], i[:n], o[:n]), want[:n], mask[:n])
    dead = cases.kind_of_ids(ids) < 0
    assert np.abs(np.nan_to_num(want[~dead & mask], posinf=0, neginf=0)).sum() > 0 and not want[dead].view(np.uint32).any()
    for per in cases.per_slot(op):                       # the selection is not the result of any single material
        assert not (cases.same_bits(per, want) | ~mask[:, None]).all()


@pytest.mark.parametrize("want_cos,op", OPS)
def test_the_permuted_table(cpu, members, main, want_cos, op):
    """same members, other slot order, a slot without material and an alias: the ids mean something else"""
    s = djb.scene(slots=cases.TABLE2, ctx=cpu, **members)
    try:
        ids, _ = cases.material_ids(len(cases.TABLE2))
        i, o = cases.eval_inputs()
        want = cases.expected(op, table=cases.TABLE2)
        mask = cases.compared(ids, i, o, cases.TABLE2)
        got = (s.evalp if want_cos else s.eval)(ids, i, o)
        cases.assert_eval(f"table 2, {op}", got, want, mask)
        none, alias = cases.TABLE2.index(None), len(cases.TABLE2) - 1
        assert (ids == none).sum() > 1000 and not np.asarray(got)[ids == none].view(np.uint32).any()
        assert (ids == alias).sum() > 1000 and np.abs(np.nan_to_num(want[ids == alias])).sum() > 0
        # the main table on these ids gives another result: the table is what decides
        other = (main.evalp if want_cos else main.eval)(ids, i, o)
        assert not (cases.same_bits(np.asarray(other), want) | ~mask[:, None]).all()
    finally:
        s.close()


@pytest.mark.parametrize("kinds", [("abc",), ("merl", "sgd"), ("utia", "sgd", "abc")])
def test_scenes_with_fewer_member_sets(cpu, members, kinds):
    absent = [k for k in cases.KINDS if k not in kinds]
    table = cases.table_without(absent)
    s = djb.scene(slots=table, ctx=cpu, **{k: members[k] for k in kinds})
    try:
        ids, _ = cases.material_ids()
        i, o = cases.eval_inputs()
        n = 8001
        got = s.evalp(ids[:n], i[:n], o[:n])
        cases.assert_eval(f"members {kinds}", got, cases.expected("evalp", table=table, n=n), cases.compared(ids, i, o, table)[:n])
        assert s.members == tuple(cases.COUNTS[k] if k in kinds else 0 for k in cases.KINDS)
    finally:
        s.close()


def test_facade_class_equals_the_members_own_eval(tmp_path):
    src = os.path.join(ROOT, "tests", "api", "scene_facade.cpp")
    exe = tmp_path / "scene_facade"
    r = subprocess.run(["g++", "-O1", "-std=c++14", "-DNVERBOSE", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), src, "-L" + LIBDIR, "-ldjb_hip",
                        "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], env=dict(os.environ, DJB_DEVICE="cpu", DJB_QUIET="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hits checked" in out.stdout and " 0 differ" in out.stdout, out.stdout


# ------------------------------------------------------------------ the C ABI's refusals
def _create(ctx, members, slots, n=None, null_slots=False, null_out=False):
    lib = _lib.load()
    table = (_lib.SceneSlot * max(len(slots), 1))()
    for k, (kind, local) in enumerate(slots):
        table[k].kind, table[k].local = KIND_VALUE.get(kind, kind), local
    h = C.c_void_p()
    ptr = lambda k: getattr(getattr(members.get(k), "_h", None), "value", None)
    st = lib.djb_scene_create(ctx._h if ctx else None, ptr("merl"), ptr("utia"), ptr("sgd"), ptr("abc"), C.c_int(len(slots) if n is None else n),
                              None if null_slots else table, None if null_out else C.byref(h))
    msg = lib.djb_last_error().decode(errors="replace")
    if st == 0:
        lib.djb_scene_destroy(h)
    return st, msg


def test_refusals(cpu, members, main):
    one = [("merl", 0)]
    for kw in (dict(null_slots=True), dict(null_out=True)):
        st, msg = _create(cpu, members, one, **kw)
        assert st == INVALID and "null argument" in msg, (st, msg)
    st, msg = _create(None, members, one)
    assert st == INVALID and "null argument" in msg, (st, msg)
    st, msg = _create(cpu, {}, one)
    assert st == INVALID and "at least one member set" in msg, (st, msg)
    for n in (0, cases.SCENE_MAX_SLOTS + 1):
        st, msg = _create(cpu, members, one, n=n)
        assert st == INVALID and "1 .. 1048576" in msg, (st, msg)
    st, msg = _create(cpu, members, one + [("merl", 2), ("merl", 3)])                 # local out of range
    assert st == INVALID and "slot 2" in msg and "outside" in msg, (st, msg)
    st, msg = _create(cpu, members, one + [("sgd", -2)])
    assert st == INVALID and "slot 1" in msg and "outside" in msg, (st, msg)
    st, msg = _create(cpu, {"merl": members["merl"]}, one + [("utia", 0)])            # a slot naming an absent set
    assert st == INVALID and "slot 1" in msg and "no utia set" in msg, (st, msg)
    st, msg = _create(cpu, members, one + [(5, 0)])                                   # DJB_KIND_LAMBERT
    assert st == INVALID and "slot 1" in msg and "kind 5" in msg, (st, msg)
    st, msg = _create(cpu, dict(members, abc=members["sgd"]), one)                    # an sgd model set passed as abc
    assert st == INVALID and "abc member" in msg, (st, msg)
    st, msg = _create(cpu, dict(members, sgd=members["abc"]), one)
    assert st == INVALID and "sgd member" in msg, (st, msg)
    st, msg = _create(cpu, members, one + [(-1, 12345), ("merl", 0)])                 # a slot without material; two slots on one material
    assert st == 0, msg
    other = djb.Context("cpu")
    st, msg = _create(other, members, one)                                            # members of another context
    assert st == INVALID and "another context" in msg, (st, msg)
    with pytest.raises(djb.exc) as e:
        djb.scene(merl=members["merl"], slots=[("velvet", 0)], ctx=cpu)
    assert e.value.status == INVALID and "slot 0" in str(e.value)
    # the batch call
    lib = _lib.load()
    n = 4
    d = np.tile(np.float32([[0.3, 0.1, 0.9]]), (n, 1)); ids = np.zeros(n, np.int32); out = np.zeros((n, 3), np.float32)
    vd, vout = djb._Vec(d), djb._Vec(out)

    def call(ctx, s, material=True, output=True):
        st = lib.djb_scene_eval_batch(ctx._h if ctx else None, s._h if s else None, C.c_int64(n), C.c_void_p(ids.ctypes.data) if material else None,
                                      C.byref(vd.view), C.byref(vd.view), C.c_int(1), C.byref(vout.view) if output else None, C.c_int(_lib.MEM_HOST))
        return st, lib.djb_last_error().decode(errors="replace")
    st, msg = call(cpu, None)
    assert st == INVALID and "null scene" in msg, (st, msg)
    st, msg = call(None, main)
    assert st == INVALID and "null ctx" in msg, (st, msg)
    st, msg = call(other, main)                                                       # a scene of another context
    assert st == INVALID and "another context" in msg, (st, msg)
    st, msg = call(cpu, main, output=False)
    assert st == INVALID and "null output" in msg, (st, msg)
    st, msg = call(cpu, main, material=False)
    assert st == INVALID and "null material" in msg, (st, msg)
    st, msg = call(cpu, main)
    assert st == 0 and np.abs(out).sum() > 0, msg
    other.close()
