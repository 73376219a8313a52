"""SGD / ABC model sets on the GPU (djb_kernels_model_set.hip): eval / evalp of hits on M resident parameter rows against the oracle's
per-material results selected by id (tests/model_set_cases.py) -- bits equal in host, dense and strided layouts and at the sizes where a
tile bound can go wrong --, rows in LDS and rows in global memory, the exact-only set, DJB_MODEL_SET_MAX rows, the 100 published rows,
a second grid-stride trip, dead waves, graph capture, in-place calls and sets of other contexts.

Every output buffer is one unit longer than the batch and the extra unit is checked after the call."""
import ctypes as C
import os

import numpy as np
import pytest

import model_set_cases as cases
from dj_brdf_amd import _lib, djb, synth
from hit_calls import Arrays, dev, graph_replay, loads, resident, view

pytestmark = pytest.mark.gpu
PREFIXES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025)
LAYOUTS = ("host", "dense", "strided")
OPS = ((0, "eval"), (1, "evalp"))
GRID_CAP = 256 * 16            # workgroups: GRID_CAP of djb_kernels_model_set.hip (launch_set), as k_eval's for these kinds


@pytest.fixture(scope="module")
def sets(gpu_ctx):
    """the main set of each kind, built from brdf objects that are closed before the first call"""
    out = {}
    for kind in cases.KINDS:
        cls = djb.sgd if kind == "sgd" else djb.abc
        members = [cls.from_params(r, ctx=gpu_ctx) for r in cases.rows(kind)]
        out[kind] = djb.model_set(members, ctx=gpu_ctx)
        for b in members:
            b.close()
        assert out[kind].n_materials == cases.M and out[kind].kind == kind
    yield out
    for s in out.values():
        s.close()


def _call(s, ids, i, o, want_cos, layout, ctx=None, over=None):
    """one call through the C ABI -> [n, 3]; over = "i" / "o": the output arrays are that input's arrays"""
    ctx = ctx or s.ctx
    A = Arrays(ctx, len(ids), layout)
    pid, vi, vo = A.arr_in(ids, np.int32), A.vec_in(i), A.vec_in(o)
    alias = {"i": vi, "o": vo}.get(over)
    out = A.vec_out("fr") if alias is None else C.byref(alias)
    _lib.check(_lib.load().djb_model_set_eval_batch(ctx._h, s._h, C.c_int64(A.n), pid, C.byref(vi), C.byref(vo), C.c_int(want_cos), out, C.c_int(A.mem)))
    return A.results("eval")["fr"] if alias is None else A.read(alias)


# ------------------------------------------------------------------ 1. bits equal to the oracle selection
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("want_cos,op", OPS)
def test_eval_equals_the_oracle_selection(sets, kind, want_cos, op):
    s = sets[kind]
    ids, bulk = cases.material_ids()
    cases.assert_ids_cover_every_class(ids, bulk, cases.M)
    cases.assert_rows_mix_the_tiers()
    i, o = cases.eval_inputs()
    want = cases.expected_eval(kind, op)
    for layout in LAYOUTS:
        cases.assert_eval(f"{kind} {op}, {layout}, n = {cases.N}", _call(s, ids, i, o, want_cos, layout), want)
    for n in PREFIXES:                     # units are independent: a prefix has the prefix's results
        for layout in ("dense", "strided"):
            cases.assert_eval(f"{kind} {op}, {layout}, n = {n}", _call(s, ids[:n], i[:n], o[:n], want_cos, layout), want[:n])
    for per in cases.eval_per_material(kind, op):
        assert not cases.same_bits(per, want).all()


# ------------------------------------------------------------------ 2. the wall block: rows in LDS, rows in global memory, the exact chains only
@pytest.mark.parametrize("kind,setting", [(k, s) for k in cases.KINDS for s in ("default", "rows global", "sgd fast off", "contract 1e-5")
                                          if k == "sgd" or s != "sgd fast off"])          # DJB_SGD_FAST concerns sgd rows alone
def test_wall_block(gpu_ctx, sets, kind, setting):
    cases.assert_wall_block_is_at_the_wall()
    ids, i, o = cases.wall_block(kind)
    s, made = sets[kind], None
    before = os.environ.get("DJB_SGD_FAST")
    try:
        if setting == "rows global":
            djb.set_model_set_rows_global(gpu_ctx, True)
        elif setting == "contract 1e-5":
            djb.set_contract_1e5(gpu_ctx, True)
        elif setting == "sgd fast off":               # read at creation: every row of this set runs the exact chains only
            os.environ["DJB_SGD_FAST"] = "0"
            s = made = djb.model_set.from_rows(kind, cases.rows(kind), ctx=gpu_ctx)
            os.environ.pop("DJB_SGD_FAST")
        for want_cos, op in OPS:
            want = cases.wall_expected(kind, op)
            for layout in ("dense", "strided"):
                got = _call(s, ids, i, o, want_cos, layout)
                cases.assert_eval(f"wall block, {kind}, {setting}, {op}, {layout}", got, want)
                assert not got[~cases.active(ids, cases.M)].view(np.uint32).any()
                if made is not None:
                    assert cases.same_bits(got, _call(sets[kind], ids, i, o, want_cos, layout)).all()
    finally:
        if before is None:
            os.environ.pop("DJB_SGD_FAST", None)
        else:
            os.environ["DJB_SGD_FAST"] = before
        djb.set_model_set_rows_global(gpu_ctx, False)
        djb.set_contract_1e5(gpu_ctx, False)
        if made is not None:
            made.close()


# ------------------------------------------------------------------ 3. the upper end: DJB_MODEL_SET_MAX rows, read from global memory
@pytest.mark.parametrize("kind", cases.KINDS)
def test_upper_end(gpu_ctx, kind):
    MAX = cases.MODEL_SET_MAX
    at = {0: 0, 1: 1, MAX // 2: (MAX // 2) % cases.M, MAX - 1: (MAX - 1) % cases.M}      # id -> row of the main set, cycled
    assert len(set(at.values())) == 4
    s = djb.model_set.from_rows(kind, cases.rows(kind)[np.arange(MAX) % cases.M], ctx=gpu_ctx)
    try:
        assert s.n_materials == MAX
        _, i, o = cases.wall_block(kind)
        n = len(i)
        ids = np.int32([0, 1, MAX // 2, MAX - 1, MAX, -1])[np.arange(n) % 6]
        per = cases.wall_per_material(kind, "evalp")
        want = np.zeros((n, 3), np.float32)
        for e, k in at.items():
            want[ids == e] = per[k][ids == e]
        for layout in ("dense", "strided", "host"):
            cases.assert_eval(f"{MAX} rows, {kind}, {layout}", _call(s, ids, i, o, 1, layout), want)
    finally:
        s.close()


# ------------------------------------------------------------------ 4. the 100 published rows
@pytest.mark.parametrize("kind", cases.KINDS)
def test_the_hundred_published_rows(gpu_ctx, kind):
    s = djb.model_set.from_names(kind, synth.MERL_NAMES, ctx=gpu_ctx)
    try:
        assert s.n_materials == 100
        i, o = cases.eval_inputs()
        cases.assert_eval(f"published rows, {kind}", _call(s, cases.published_ids(), i, o, 1, "dense"), cases.published_expected(kind, "evalp"))
    finally:
        s.close()


# ------------------------------------------------------------------ 5. a second, ragged grid-stride trip
@pytest.mark.parametrize("kind", cases.KINDS)
def test_second_grid_stride_trip(sets, kind):
    """GRID_CAP workgroups cover GRID_CAP * 256 hits; the 4 096 - 179 behind them send sixteen workgroups on a second trip, the last one ragged"""
    ids, i, o = cases.wall_block(kind)
    n = GRID_CAP * 256 + 4096 - 179
    reps = -(-n // len(ids))
    tile = lambda a: np.ascontiguousarray(np.concatenate([a] * reps)[:n])
    want = tile(cases.wall_expected(kind, "evalp"))
    got = _call(sets[kind], tile(ids), tile(i), tile(o), 1, "dense")
    cases.assert_eval(f"second trip, {kind}", got, want)


# ------------------------------------------------------------------ 6. a wave of dead hits, all-dead batches
@pytest.mark.parametrize("n", [64, 300])
def test_all_dead_batches(sets, n):
    for kind in cases.KINDS:
        _, i, o = cases.wall_block(kind)
        ids = cases.inactive_values(cases.M)[np.arange(n) % 5]
        for layout in LAYOUTS:
            for want_cos in (0, 1):
                assert not _call(sets[kind], ids, i[:n], o[:n], want_cos, layout).view(np.uint32).any()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_a_wave_of_dead_hits_among_live_ones(sets, kind):
    ids, i, o = (a.copy() for a in cases.wall_block(kind))
    ids[64:128] = -1                                  # one whole wave of the first workgroup
    ids[256 + 192:512] = cases.M                      # the last wave of the second
    want = cases.wall_expected(kind, "eval").copy()
    want[~cases.active(ids, cases.M)] = 0
    cases.assert_eval(f"dead waves, {kind}", _call(sets[kind], ids, i, o, 0, "dense"), want)


# ------------------------------------------------------------------ 7. graph capture
def test_calls_replay_from_a_captured_graph(gpu_ctx, sets):
    import torch
    lib = _lib.load()
    gids, gi, go = cases.wall_block("sgd")
    n = len(gids)
    ids2, _ = cases.material_ids()
    i2, o2 = cases.eval_inputs()
    data = [(gids, gi, go), (ids2[:n], i2[:n], o2[:n])]
    ids, i, o = (resident(gpu_ctx, a) for a in data[0])
    outs = [torch.zeros((3, n), dtype=torch.float32, device=dev(gpu_ctx)) for _ in range(4)]
    vi, vo = view(i.data_ptr(), n, "dense"), view(o.data_ptr(), n, "dense")
    vouts = [view(a.data_ptr(), n, "dense") for a in outs]

    def launch():                           # four device-memory calls: sgd eval, sgd evalp, abc eval, abc evalp
        for k, vout in enumerate(vouts):
            _lib.check(lib.djb_model_set_eval_batch(gpu_ctx._h, sets[cases.KINDS[k >> 1]]._h, C.c_int64(n), C.c_void_p(ids.data_ptr()), C.byref(vi), C.byref(vo),
                                                    C.c_int(k & 1), C.byref(vout), C.c_int(_lib.MEM_DEVICE)))
    want = graph_replay(gpu_ctx, launch, outs, loads(gpu_ctx, (ids, i, o), data))
    assert want[0][1].abs().sum() > 0 and not torch.equal(want[0][1], want[1][1])
    cases.assert_eval("eager, sgd evalp", want[0][1].cpu().numpy().T, cases.wall_expected("sgd", "evalp"))


# ------------------------------------------------------------------ 8. aliasing
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("layout", ["dense", "strided"])
def test_in_place_call_equals_out_of_place(gpu_ctx, sets, kind, layout):
    ids, i, o = cases.wall_block(kind)
    want = _call(sets[kind], ids, i, o, 1, layout)
    for which in ("i", "o"):
        got = _call(sets[kind], ids, i, o, 1, layout, over=which)      # the output arrays are i's (o's) arrays
        cases.assert_eval(f"in place over {which}, {kind}, {layout}", got, want)
        cases.assert_eval(f"in place over {which}, {kind}, {layout}, against the oracle", got, cases.wall_expected(kind, "evalp"))


# ------------------------------------------------------------------ 9. contexts
def test_a_set_of_another_context_is_refused(gpu_ctx, sets):
    lib = _lib.load()
    ids, i, o = cases.wall_block("sgd")
    other = djb.Context(gpu_ctx.device)
    cpu = djb.cpu_context()
    for ctx, layout, what in ((other, "host", "another context"), (other, "dense", "another context"), (cpu, "host", "different back ends")):
        with pytest.raises(djb.exc) as e:
            _call(sets["sgd"], ids[:300], i[:300], o[:300], 0, layout, ctx=ctx)
        assert e.value.status == 1 and what in str(e.value), str(e.value)
    foreign = djb.sgd.from_params(cases.rows("sgd")[1], ctx=other)
    ptrs = (C.c_void_p * 1)(foreign._h.value)
    out = C.c_void_p()
    st = lib.djb_model_set_create_from_brdfs(gpu_ctx._h, C.c_int(1), ptrs, C.byref(out))
    assert st == 1 and "another context" in lib.djb_last_error().decode(errors="replace")
    cases.assert_eval("own context", _call(sets["sgd"], ids[:300], i[:300], o[:300], 0, "dense"), cases.wall_expected("sgd", "eval")[:300])
