"""The fitted tabular proxies of SGD / ABC model sets on the host path (CPU context): djb.model_set.fit_proxy / .proxy_info / .proxy_tables /
.evalp_is_proxy / .evalp_pdf_proxy against the oracle's per-material fits and compositions selected by id (tests/model_set_proxy_cases.py) --
the main set, the tables, the refit, the degenerate row, the refusals of the C ABI -- and what the case module says of its own values.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import model_set_proxy_cases as cases
import trip_cases
from dj_brdf_amd import _lib, djb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dj_brdf_amd", "lib")
INVALID = 1
N = cases.HOST_N


@pytest.fixture(scope="module")
def cpu():
    return djb.cpu_context()


@pytest.fixture(scope="module")
def sets(cpu):
    """the main set of each kind with the main fit (res 90, shadow on)"""
    out = {kind: djb.model_set.from_rows(kind, cases.rows(kind), ctx=cpu) for kind in cases.KINDS}
    for s in out.values():
        assert s.proxy_info() == (0, False)
        s.fit_proxy()
        assert s.proxy_info() == (90, True)
    yield out
    for s in out.values():
        s.close()


def test_the_cases_are_what_the_module_says():
    for res, shadow in cases.FITS:
        cases.assert_conditions(res, shadow, N)
    ids = cases.alternating_ids()
    assert len(ids) == 4096 and (ids[0::3] == 0).all() and (ids[1::3] == cases.DEGENERATE[1]).all() and not cases.active(ids[2::3], cases.M).any()
    big = cases.big_ids()
    assert big.max() > cases.BIG_M and cases.BIG_M - 1 in big and (cases.fold(big) < cases.M).all() and len(set(big[cases.active(big, cases.BIG_M)])) == cases.BIG_M


def test_the_trip_size_is_the_launch_codes():
    """grid_capped(n, BLOCK, GRID_CAP) workgroups of BLOCK hits (djb_kernels_model_set_proxy.hip: Launch): the batch of the second-trip
    test sends sixteen workgroups on a second trip, the last one ragged"""
    n = cases.TRIP_N
    assert trip_cases.grid_capped(n, cases.BLOCK, cases.GRID_CAP) * cases.BLOCK == cases.TRIP == 4096 * 256 == 1_048_576
    assert n == cases.TRIP + trip_cases.BLOCK_N - trip_cases.RAGGED and n - cases.TRIP == 15 * 256 + 77


@pytest.mark.parametrize("kind", cases.KINDS)
def test_tables_equal_the_oracles_fits(sets, kind):
    for m in range(cases.M):
        cases.assert_tables(f"{kind}, material {m}", sets[kind].proxy_tables(m), kind, m, 90, True)
    assert len(sets["sgd"].proxy_tables(cases.DEGENERATE[1])["qf"]) == 2


@pytest.mark.parametrize("kind", cases.KINDS)
def test_the_single_material_tabular_of_every_row_equals_the_oracles(cpu, kind):
    """what the set is held against exists already: tabular(model(row), 90) of the product, the degenerate row included"""
    for m, row in enumerate(cases.rows(kind)):
        b = (djb.sgd if kind == "sgd" else djb.abc).from_params(row, ctx=cpu)
        t = djb.tabular(b, 90, True, ctx=cpu)
        cases.assert_tables(f"single {kind} {m}", {"p22": t.get_p22v(), "sigma": t.get_sigmav(), "qf": t.get_qfv()}, kind, m, 90, True)
        t.close(); b.close()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_sampling_equals_the_oracle_selection(sets, kind):
    o, u1, u2 = cases.sampler_inputs(N)
    ids = cases.material_ids(N)
    want = cases.expected_sample(kind, n=N)
    for n in (N, 1, 2, 97):
        cases.assert_same(f"{kind} sampling, n = {n}", sets[kind].evalp_is_proxy(ids[:n], u1[:n], u2[:n], o[:n]), tuple(a[:n] for a in want))
    act = cases.active(ids, cases.M)
    assert not any(a[~act].view(np.uint32).any() for a in want) and np.abs(np.nan_to_num(want[0][act], posinf=0, neginf=0)).sum() > 0
    for per in cases.sample_per_material(kind, 90, True, N):       # the selection is not the result of any single material
        assert not cases.same_bits(per[1], want[1]).all()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_light_sample_equals_the_oracle_selection(sets, kind):
    i, o = cases.light_inputs()                                   # all cases.N pairs: the host path takes them in milliseconds
    ids = cases.material_ids()
    want = cases.expected_light(kind)
    for n in (cases.N, 1, 2, 97):
        cases.assert_light(f"{kind} light sample, n = {n}", sets[kind].evalp_pdf_proxy(ids[:n], i[:n], o[:n]), tuple(a[:n] for a in want))
    guard = (i[:, 2] <= 0) | (o[:, 2] <= 0)
    assert guard.sum() > 1000 and not any(a[guard].view(np.uint32).any() for a in want) and (want[1] > 0).sum() > cases.N // 2
    for per in cases.light_per_material(kind, 90, True):
        assert not cases.same_bits(per[1], want[1]).all()


def test_the_degenerate_row_next_to_a_regular_one(sets):
    """ids alternate row 0 / row 5 (n_qf = 2, non-finite tables, pdf 0) / dead on every hit"""
    ids, (o, u1, u2), want, (i, o2), want_light = cases.alternating_case()
    n = len(ids)
    cases.assert_same("degenerate row, sampling", sets["sgd"].evalp_is_proxy(ids, u1, u2, o), want)
    deg = ids == cases.DEGENERATE[1]
    assert not want[2][deg].view(np.uint32).any() and not np.isfinite(want[0][deg]).all() and (want[2][ids == 0] > 0).sum() > n // 8
    cases.assert_light("degenerate row, light sample", sets["sgd"].evalp_pdf_proxy(ids, i, o2), want_light)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_a_refit_replaces_the_first_fit(cpu, kind):
    s = djb.model_set.from_rows(kind, cases.rows(kind), ctx=cpu)
    try:
        s.fit_proxy()
        res, shadow = cases.FITS[1]
        s.fit_proxy(res, shadow=shadow)
        assert s.proxy_info() == (res, shadow)
        for m in range(cases.M):
            cases.assert_tables(f"refit {kind} {m}", s.proxy_tables(m), kind, m, res, shadow)
        ids = cases.material_ids(N)
        o, u1, u2 = cases.sampler_inputs(N)
        cases.assert_same(f"refit {kind}, sampling", s.evalp_is_proxy(ids, u1, u2, o), cases.expected_sample(kind, res, shadow, N))
        i, o2 = cases.light_inputs()
        want = cases.expected_light(kind, res, shadow)
        cases.assert_light(f"refit {kind}, light sample", s.evalp_pdf_proxy(cases.material_ids(), i, o2), want)
        assert not cases.same_bits(want[1], cases.expected_light(kind)[1]).all()             # another fit, other values
    finally:
        s.close()


def test_facade_class_equals_the_single_material_route(tmp_path):
    src = os.path.join(ROOT, "tests", "api", "model_set_proxy_facade.cpp")
    exe = tmp_path / "model_set_proxy_facade"
    r = subprocess.run(["g++", "-O1", "-std=c++14", "-DNVERBOSE", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), src, "-L" + LIBDIR, "-ldjb_hip",
                        "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], env=dict(os.environ, DJB_DEVICE="cpu", DJB_QUIET="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "values checked" in out.stdout and " 0 differ" in out.stdout, out.stdout


# ------------------------------------------------------------------ refusals: the status, the message, nothing written
def test_refusals(cpu, sets):
    cases.assert_refusals(cpu, sets["sgd"], djb.Context("cpu"))


def test_the_entry_bound_on_materials_times_resolution(cpu):
    """M * res <= DJB_MODEL_SET_PROXY_MAX_ENTRIES is checked before anything is fitted"""
    lib = _lib.load()
    s = djb.model_set.from_rows("abc", cases.rows("abc")[np.arange(65536) % cases.M], ctx=cpu)
    try:
        st = lib.djb_model_set_fit_proxy(cpu._h, s._h, cases.PROXY_MAX_ENTRIES // 65536 + 1, 1)
        assert st == INVALID and "table entries" in lib.djb_last_error().decode() and s.proxy_info() == (0, False)
    finally:
        s.close()
