"""The fitted tabular proxies of SGD / ABC model sets on the GPU (djb_kernels_model_set_proxy.hip, djb_model_set_fit_proxy): the fit of every
row on the device, the sampling step and the light sample per hit against the oracle's per-material fits and compositions selected by id
(tests/model_set_proxy_cases.py) -- bits equal in host, dense and strided layouts and at the sizes where a tile bound can go wrong --, rows
in LDS and in global memory, the exact-only set, the refit, 300 materials fitted in three chunks, the degenerate row in mixed waves, a
second grid-stride trip, dead and guarded hits, graph capture and the refusals.

Every output buffer is one unit longer than the batch and the extra unit is checked after the call."""
import ctypes as C
import os

import numpy as np
import pytest

import model_set_cases
import model_set_proxy_cases as cases
from dj_brdf_amd import _lib, djb
from hit_calls import Arrays, dev, graph_replay, loads, resident, view

pytestmark = pytest.mark.gpu
LAYOUTS = ("host", "dense", "strided")


@pytest.fixture(scope="module")
def sets(gpu_ctx):
    """the main set of each kind with the main fit (res 90, shadow on)"""
    out = {kind: djb.model_set.from_rows(kind, cases.rows(kind), ctx=gpu_ctx) for kind in cases.KINDS}
    for s in out.values():
        assert s.proxy_info() == (0, False)
        s.fit_proxy()
        assert s.proxy_info() == (90, True)
    yield out
    for s in out.values():
        s.close()


def _sample(s, ids, u1, u2, o, layout, ctx=None):
    """djb_model_set_evalp_is_proxy_batch through the C ABI -> (weight, i, pdf)"""
    ctx = ctx or s.ctx
    A = Arrays(ctx, len(ids), layout)
    vo = A.vec_in(o)
    _lib.check(_lib.load().djb_model_set_evalp_is_proxy_batch(ctx._h, s._h, C.c_int64(A.n), A.arr_in(ids, np.int32), A.arr_in(u1), A.arr_in(u2), C.byref(vo),
                                                             A.vec_out("weight"), A.vec_out("i"), A.arr_out("pdf"), C.c_int(A.mem)))
    return tuple(A.results("sampling").values())


def _light(s, ids, i, o, layout, ctx=None):
    """djb_model_set_evalp_pdf_proxy_batch through the C ABI -> (fr, pdf)"""
    ctx = ctx or s.ctx
    A = Arrays(ctx, len(ids), layout)
    vi, vo = A.vec_in(i), A.vec_in(o)
    _lib.check(_lib.load().djb_model_set_evalp_pdf_proxy_batch(ctx._h, s._h, C.c_int64(A.n), A.arr_in(ids, np.int32), C.byref(vi), C.byref(vo), A.vec_out("fr"),
                                                              A.arr_out("pdf"), C.c_int(A.mem)))
    return tuple(A.results("light sample").values())


def _head(arrays, n):
    return tuple(a[:n] for a in arrays)


# ------------------------------------------------------------------ 1. the fit on the device
@pytest.mark.parametrize("kind", cases.KINDS)
def test_tables_equal_the_oracles_fits(sets, kind):
    for m in range(cases.M):
        cases.assert_tables(f"{kind}, material {m}", sets[kind].proxy_tables(m), kind, m, 90, True)
    assert len(sets["sgd"].proxy_tables(cases.DEGENERATE[1])["qf"]) == 2


# ------------------------------------------------------------------ 2. the main set: bits equal to the oracle selection
@pytest.mark.parametrize("kind", cases.KINDS)
def test_sampling_equals_the_oracle_selection(sets, kind):
    cases.assert_conditions()
    o, u1, u2 = cases.sampler_inputs()
    ids = cases.material_ids()
    want = cases.expected_sample(kind)
    for layout in LAYOUTS:
        cases.assert_same(f"{kind} sampling, {layout}", _sample(sets[kind], ids, u1, u2, o, layout), want)
    for n in cases.RAGGED:                  # units are independent: a prefix has the prefix's results
        for layout in ("dense", "strided"):
            cases.assert_same(f"{kind} sampling, {layout}, n = {n}", _sample(sets[kind], ids[:n], u1[:n], u2[:n], o[:n], layout), _head(want, n))
    for per in cases.sample_per_material(kind, 90, True):
        assert not cases.same_bits(per[1], want[1]).all()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_light_sample_equals_the_oracle_selection(sets, kind):
    i, o = cases.light_inputs()
    ids = cases.material_ids()
    want = cases.expected_light(kind)
    for layout in LAYOUTS:
        cases.assert_light(f"{kind} light sample, {layout}", _light(sets[kind], ids, i, o, layout), want)
    for n in cases.RAGGED:
        for layout in ("dense", "strided"):
            cases.assert_light(f"{kind} light sample, {layout}, n = {n}", _light(sets[kind], ids[:n], i[:n], o[:n], layout), _head(want, n))
    for per in cases.light_per_material(kind, 90, True):
        assert not cases.same_bits(per[1], want[1]).all()


@pytest.mark.parametrize("kind,setting", [(k, s) for k in cases.KINDS for s in ("rows global", "sgd fast off", "contract 1e-5")
                                          if k == "sgd" or s != "sgd fast off"])          # DJB_SGD_FAST concerns sgd rows alone
def test_main_set_under_the_settings(gpu_ctx, sets, kind, setting):
    s, made = sets[kind], None
    before = os.environ.get("DJB_SGD_FAST")
    try:
        if setting == "rows global":
            djb.set_model_set_rows_global(gpu_ctx, True)
        elif setting == "contract 1e-5":
            djb.set_contract_1e5(gpu_ctx, True)
        else:                                         # read at creation: every row of this set runs the exact chains only
            os.environ["DJB_SGD_FAST"] = "0"
            s = made = djb.model_set.from_rows(kind, cases.rows(kind), ctx=gpu_ctx)
            os.environ.pop("DJB_SGD_FAST")
            s.fit_proxy()
            for m in range(cases.M):
                cases.assert_tables(f"{setting}, material {m}", s.proxy_tables(m), kind, m, 90, True)
        ids = cases.material_ids()
        for layout in ("dense", "strided"):
            cases.assert_same(f"{kind} sampling, {setting}, {layout}", _sample(s, ids, *cases.sampler_inputs()[1:], cases.sampler_inputs()[0], layout),
                              cases.expected_sample(kind))
            cases.assert_light(f"{kind} light sample, {setting}, {layout}", _light(s, ids, *cases.light_inputs(), layout), cases.expected_light(kind))
    finally:
        if before is None:
            os.environ.pop("DJB_SGD_FAST", None)
        else:
            os.environ["DJB_SGD_FAST"] = before
        djb.set_model_set_rows_global(gpu_ctx, False)
        djb.set_contract_1e5(gpu_ctx, False)
        if made is not None:
            made.close()


# ------------------------------------------------------------------ 3. the refit
@pytest.mark.parametrize("kind", cases.KINDS)
def test_a_refit_replaces_the_first_fit(gpu_ctx, kind):
    s = djb.model_set.from_rows(kind, cases.rows(kind), ctx=gpu_ctx)
    try:
        s.fit_proxy()
        res, shadow = cases.FITS[1]
        s.fit_proxy(res, shadow=shadow)
        assert s.proxy_info() == (res, shadow)
        for m in range(cases.M):
            cases.assert_tables(f"refit {kind} {m}", s.proxy_tables(m), kind, m, res, shadow)
        ids = cases.material_ids()
        o, u1, u2 = cases.sampler_inputs()
        want = cases.expected_light(kind, res, shadow)
        for layout in ("dense", "strided"):
            cases.assert_same(f"refit {kind}, sampling, {layout}", _sample(s, ids, u1, u2, o, layout), cases.expected_sample(kind, res, shadow))
            cases.assert_light(f"refit {kind}, light sample, {layout}", _light(s, ids, *cases.light_inputs(), layout), want)
        assert not cases.same_bits(want[1], cases.expected_light(kind)[1]).all()
    finally:
        s.close()


# ------------------------------------------------------------------ 4. offsets and chunking: 300 materials, fitted 128 at a time
@pytest.mark.parametrize("kind", cases.KINDS)
def test_three_hundred_materials(gpu_ctx, sets, kind):
    """material m holds row m % 6: its tables are, bit for bit, those of that row in the six-material set -- the fit does not depend on the
    chunk a material is fitted in -- and its hits get that row's results; rows are read from global memory (above both LDS budgets)"""
    s = djb.model_set.from_rows(kind, cases.big_rows(kind), ctx=gpu_ctx)
    try:
        s.fit_proxy()
        assert s.n_materials == cases.BIG_M and s.proxy_info() == (90, True)
        small = [sets[kind].proxy_tables(m) for m in range(cases.M)]
        for m in range(cases.BIG_M):
            t = s.proxy_tables(m)
            for name in ("p22", "sigma", "qf"):
                assert t[name].shape == small[m % cases.M][name].shape and cases.same_bits(t[name], small[m % cases.M][name]).all(), (m, name)
        for m in (0, 127, 128, 255, 256, cases.BIG_M - 1):                           # the ends of the three chunks, against the oracle itself
            cases.assert_tables(f"{kind}, material {m} of {cases.BIG_M}", s.proxy_tables(m), kind, m, 90, True)
        ids = cases.big_ids()
        folded = cases.fold(ids)
        o, u1, u2 = cases.sampler_inputs()
        for layout in ("dense", "strided"):
            cases.assert_same(f"{cases.BIG_M} materials, {kind}, sampling, {layout}", _sample(s, ids, u1, u2, o, layout), cases.expected_sample(kind, ids=folded))
            cases.assert_light(f"{cases.BIG_M} materials, {kind}, light sample, {layout}", _light(s, ids, *cases.light_inputs(), layout),
                               cases.expected_light(kind, ids=folded))
    finally:
        s.close()


# ------------------------------------------------------------------ 5. mixed waves, the degenerate row
@pytest.mark.parametrize("kind", cases.KINDS)
def test_mixed_waves(sets, kind):
    """model_set_cases.wall_block's id pattern on sampler inputs: the id changes with every active hit, every third hit is dead"""
    ids = cases.wall_ids(kind)
    n = len(ids)
    o, u1, u2 = _head(cases.sampler_inputs(), n)
    i, o2 = _head(cases.light_inputs(), n)
    for layout in ("dense", "strided"):
        got = _sample(sets[kind], ids, u1, u2, o, layout)
        cases.assert_same(f"mixed waves, {kind}, sampling, {layout}", got,
                          cases.select_all([_head(r, n) for r in cases.sample_per_material(kind, 90, True)], ids))
        assert not any(a[2::3].view(np.uint32).any() for a in got)
        cases.assert_light(f"mixed waves, {kind}, light sample, {layout}", _light(sets[kind], ids, i, o2, layout),
                           cases.select_all([_head(r, n) for r in cases.light_per_material(kind, 90, True)], ids))


def test_the_degenerate_row_next_to_a_regular_one(sets):
    """ids alternate row 0 / row 5 (n_qf = 2, non-finite tables, pdf 0) / dead on every hit: every wave mixes n_qf = 90 with n_qf = 2"""
    ids, (o, u1, u2), want, (i, o2), want_light = cases.alternating_case()
    deg = ids == cases.DEGENERATE[1]
    assert not want[2][deg].view(np.uint32).any() and not np.isfinite(want[0][deg]).all() and (want[2][ids == 0] > 0).sum() > len(ids) // 8
    for layout in LAYOUTS:
        cases.assert_same(f"degenerate row, sampling, {layout}", _sample(sets["sgd"], ids, u1, u2, o, layout), want)
        cases.assert_light(f"degenerate row, light sample, {layout}", _light(sets["sgd"], ids, i, o2, layout), want_light)


# ------------------------------------------------------------------ 6. a second, ragged grid-stride trip
@pytest.mark.parametrize("kind", cases.KINDS)
def test_second_grid_stride_trip(sets, kind):
    """GRID_CAP workgroups cover TRIP hits; the 4 096 - 179 behind them send sixteen workgroups on a second trip, the last one ragged"""
    ids = cases.wall_ids(kind)
    b = len(ids)
    n = cases.TRIP_N
    t = lambda a: cases.tiled(a, n)
    o, u1, u2 = _head(cases.sampler_inputs(), b)
    want = cases.select_all([_head(r, b) for r in cases.sample_per_material(kind, 90, True)], ids)
    cases.assert_same(f"second trip, {kind}, sampling", _sample(sets[kind], t(ids), t(u1), t(u2), t(o), "dense"), tuple(t(a) for a in want))
    i, o2 = _head(cases.light_inputs(), b)
    want = cases.select_all([_head(r, b) for r in cases.light_per_material(kind, 90, True)], ids)
    assert (want[1][cases.TRIP % b:][:4096 - 179] > 0).sum() > 1000                   # the second trip is not vacuous
    cases.assert_light(f"second trip, {kind}, light sample", _light(sets[kind], t(ids), t(i), t(o2), "dense"), tuple(t(a) for a in want))


# ------------------------------------------------------------------ 7. dead and guarded hits
@pytest.mark.parametrize("n", [64, 300])
def test_all_dead_and_all_guarded_batches(sets, n):
    o, u1, u2 = _head(cases.sampler_inputs(), n)
    i, o2 = (np.array(a[:n]) for a in cases.light_inputs())
    dead = cases.inactive_values(cases.M)[np.arange(n) % 5]
    live = (np.arange(n) % cases.M).astype(np.int32)
    below_i, below_o = i.copy(), o2.copy()
    below_i[0::2, 2] = -np.abs(below_i[0::2, 2]); below_o[1::2, 2] = -np.abs(below_o[1::2, 2]); below_o[3::4, 2] = 0.0
    for kind in cases.KINDS:
        for layout in LAYOUTS:
            assert not any(a.view(np.uint32).any() for a in _sample(sets[kind], dead, u1, u2, o, layout))
            assert not any(a.view(np.uint32).any() for a in _light(sets[kind], dead, i, o2, layout))
            assert not any(a.view(np.uint32).any() for a in _light(sets[kind], live, below_i, below_o, layout))     # live ids, every pair guarded


@pytest.mark.parametrize("kind", cases.KINDS)
def test_a_wave_of_dead_hits_among_live_ones(sets, kind):
    ids = np.array(cases.wall_ids(kind))
    n = len(ids)
    ids[64:128] = -1                                  # one whole wave of the first workgroup
    ids[256 + 192:512] = cases.M                      # the last wave of the second
    o, u1, u2 = _head(cases.sampler_inputs(), n)
    cases.assert_same(f"dead waves, {kind}, sampling", _sample(sets[kind], ids, u1, u2, o, "dense"),
                      cases.select_all([_head(r, n) for r in cases.sample_per_material(kind, 90, True)], ids))
    i, o2 = _head(cases.light_inputs(), n)
    cases.assert_light(f"dead waves, {kind}, light sample", _light(sets[kind], ids, i, o2, "dense"),
                       cases.select_all([_head(r, n) for r in cases.light_per_material(kind, 90, True)], ids))


# ------------------------------------------------------------------ 8. graph capture
def test_calls_replay_from_a_captured_graph(gpu_ctx, sets):
    """the two calls of one bounce, captured into one graph after one warm call and replayed on new inputs"""
    import torch
    lib = _lib.load()
    n = 4096
    s = sets["sgd"]
    o_, u1_, u2_ = cases.sampler_inputs()
    li, lo = cases.light_inputs()
    data = [(cases.wall_ids("sgd"), u1_[:n], u2_[:n], o_[:n], li[:n], lo[:n]),
            (cases.material_ids()[n:2 * n], u1_[n:2 * n], u2_[n:2 * n], o_[n:2 * n], li[n:2 * n], lo[n:2 * n])]
    ids, u1, u2, o, i, o2 = (resident(gpu_ctx, a) for a in data[0])
    w, si, fr = (torch.zeros((3, n), dtype=torch.float32, device=dev(gpu_ctx)) for _ in range(3))
    spdf, lpdf = (torch.zeros(n, dtype=torch.float32, device=dev(gpu_ctx)) for _ in range(2))
    v = lambda t: view(t.data_ptr(), n, "dense")
    vo, vw, vsi, vi, vo2, vfr = v(o), v(w), v(si), v(i), v(o2), v(fr)

    def launch():
        _lib.check(lib.djb_model_set_evalp_is_proxy_batch(gpu_ctx._h, s._h, C.c_int64(n), C.c_void_p(ids.data_ptr()), C.c_void_p(u1.data_ptr()),
                                                          C.c_void_p(u2.data_ptr()), C.byref(vo), C.byref(vw), C.byref(vsi), C.c_void_p(spdf.data_ptr()),
                                                          C.c_int(_lib.MEM_DEVICE)))
        _lib.check(lib.djb_model_set_evalp_pdf_proxy_batch(gpu_ctx._h, s._h, C.c_int64(n), C.c_void_p(ids.data_ptr()), C.byref(vi), C.byref(vo2), C.byref(vfr),
                                                           C.c_void_p(lpdf.data_ptr()), C.c_int(_lib.MEM_DEVICE)))
    want = graph_replay(gpu_ctx, launch, [w, si, spdf, fr, lpdf], loads(gpu_ctx, (ids, u1, u2, o, i, o2), data))
    assert want[0][2].abs().sum() > 0 and not torch.equal(want[0][2], want[1][2])
    ids0 = data[0][0]
    cases.assert_same("eager, sampling", [want[0][0].cpu().numpy().T, want[0][1].cpu().numpy().T, want[0][2].cpu().numpy()],
                      cases.select_all([_head(r, n) for r in cases.sample_per_material("sgd", 90, True)], ids0))
    cases.assert_light("eager, light sample", [want[0][3].cpu().numpy().T, want[0][4].cpu().numpy()],
                       cases.select_all([_head(r, n) for r in cases.light_per_material("sgd", 90, True)], ids0))


# ------------------------------------------------------------------ 9. refusals
def test_refusals(gpu_ctx, sets):
    other = djb.Context(gpu_ctx.device)
    cases.assert_refusals(gpu_ctx, sets["sgd"], other)
    cases.assert_refusals(gpu_ctx, sets["sgd"], djb.cpu_context())
    ids, o, u1, u2 = cases.material_ids()[:300], *(_head(cases.sampler_inputs(), 300))
    for layout in ("host", "dense"):         # device memory too: a set of another context is refused before anything is launched
        with pytest.raises(djb.exc) as e:
            _sample(sets["sgd"], ids, u1, u2, o, layout, ctx=other)
        assert e.value.status == 1 and "another context" in str(e.value), str(e.value)
    cases.assert_same("own context", _sample(sets["sgd"], ids, u1, u2, o, "dense"), _head(cases.expected_sample("sgd"), 300))
    assert model_set_cases.MODEL_SET_MAX * 90 < cases.PROXY_MAX_ENTRIES
