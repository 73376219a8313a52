"""UTIA material sets on the GPU (djb_kernels_utia_set.hip: tier 1 + the fix kernel): eval / evalp of hits on M resident tables against
the oracle's per-material results selected by id (tests/utia_set_cases.py) -- bits equal in host, dense and strided layouts and at the
sizes where a tile bound can go wrong --, the three paths of the fix kernel, a second grid-stride trip, byte offsets beyond 2^31,
dead waves, graph capture, in-place calls and sets of other contexts.

Every output buffer is one unit longer than the batch and the extra unit is checked after the call."""
import ctypes as C

import numpy as np
import pytest

import utia_set_cases as cases
from dj_brdf_amd import _lib, djb
from hit_calls import Arrays, dev, graph_replay, loads, resident, view

pytestmark = pytest.mark.gpu
PREFIXES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025)
LAYOUTS = ("host", "dense", "strided")


@pytest.fixture(scope="module")
def uset(gpu_ctx):
    """the three-material set; its sources are destroyed before the first call"""
    members = cases.product_members(gpu_ctx)
    s = djb.utia_set(members, ctx=gpu_ctx)
    for b in members:
        b.close()
    assert s.n_materials == cases.M
    yield s
    s.close()


def _call(s, ids, i, o, want_cos, layout, ctx=None, over=None):
    """one call through the C ABI -> [n, 3]; over = "i" / "o": the output arrays are that input's arrays"""
    ctx = ctx or s.ctx
    A = Arrays(ctx, len(ids), layout)
    pid, vi, vo = A.arr_in(ids, np.int32), A.vec_in(i), A.vec_in(o)
    alias = {"i": vi, "o": vo}.get(over)
    out = A.vec_out("fr") if alias is None else C.byref(alias)
    _lib.check(_lib.load().djb_utia_set_eval_batch(ctx._h, s._h, C.c_int64(A.n), pid, C.byref(vi), C.byref(vo), C.c_int(want_cos), out, C.c_int(A.mem)))
    return A.results("eval")["fr"] if alias is None else A.read(alias)


# ------------------------------------------------------------------ 1. bits equal to the oracle selection
@pytest.mark.parametrize("want_cos", [0, 1])
def test_eval_equals_the_oracle_selection(uset, want_cos):
    ids, bulk = cases.material_ids()
    cases.assert_ids_cover_every_class(ids, bulk)
    i, o = cases.eval_inputs()
    op = "evalp" if want_cos else "eval"
    want = cases.expected_eval(op)
    mask = cases.compared(ids, i, o)
    for layout in LAYOUTS:
        cases.assert_eval(f"{op}, {layout}, n = {cases.N}", _call(uset, ids, i, o, want_cos, layout), want, mask)
    for n in PREFIXES:                     # units are independent: a prefix has the prefix's results; the cooperative fetch involves lanes past the end
        for layout in ("dense", "strided"):
            cases.assert_eval(f"{op}, {layout}, n = {n}", _call(uset, ids[:n], i[:n], o[:n], want_cos, layout), want[:n], mask[:n])
    for per in cases.eval_per_material(op):
        assert not (cases.same_bits(per, want) | ~mask[:, None]).all()


# ------------------------------------------------------------------ 2. the grid-line block: the three paths of the fix kernel
@pytest.mark.parametrize("setting", ["default", "cap 1", "cap 0", "exact only"])
def test_grid_line_block(gpu_ctx, uset, setting):
    ids, i, o = cases.grid_block()
    every = np.ones(len(ids), bool)
    try:
        if setting == "cap 1":
            djb.set_test_worklist_cap(gpu_ctx, 1)           # overflow as soon as two pairs decline
        elif setting == "cap 0":
            djb.set_test_worklist_cap(gpu_ctx, 0)           # the whole batch redone, ids honoured
        elif setting == "exact only":
            djb.set_utia_exact_only(gpu_ctx, True)
        for want_cos, op in ((0, "eval"), (1, "evalp")):
            want = cases.grid_expected(op)
            for layout in ("dense", "strided"):
                got = _call(uset, ids, i, o, want_cos, layout)
                cases.assert_eval(f"grid lines, {setting}, {op}, {layout}", got, want, every)
                assert not got[~cases.active(ids, cases.M)].view(np.uint32).any()
    finally:
        djb.set_test_worklist_cap(gpu_ctx, -1)
        djb.set_utia_exact_only(gpu_ctx, False)


# ------------------------------------------------------------------ 3. a second, ragged grid-stride trip
def test_second_grid_stride_trip(uset):
    """16 384 workgroups cover 16 384 * 256 hits; the 4 096 - 179 behind them send sixteen workgroups on a second trip, the last one ragged"""
    ids, i, o = cases.grid_block()
    n = 16384 * 256 + 4096 - 179
    reps = -(-n // len(ids))
    tile = lambda a: np.ascontiguousarray(np.concatenate([a] * reps)[:n])
    want = tile(cases.grid_expected("evalp"))
    got = _call(uset, tile(ids), tile(i), tile(o), 1, "dense")
    cases.assert_eval("second trip", got, want, np.ones(n, bool))


# ------------------------------------------------------------------ 4. the highest material: byte offsets beyond 2^31
def test_highest_material(gpu_ctx):
    """M = 256 from repeated handles, 2.7 GB: material 0 is table A, 128 and 255 are table B, the rest table C"""
    import torch
    members = cases.product_members(gpu_ctx)
    layout = [2] * 256
    layout[0] = 0; layout[128] = 1; layout[255] = 1
    s = djb.utia_set([members[k] for k in layout], ctx=gpu_ctx)
    try:
        for b in members:
            b.close()
        assert s.n_materials == 256
        gids, i, o = cases.grid_block()
        n = len(gids)
        ids = np.int32([0, 127, 128, 255, 256, -1])[np.arange(n) % 6]
        per = cases.grid_per_material("evalp")
        want = np.zeros((n, 3), np.float32)
        for e, k in ((0, 0), (127, 2), (128, 1), (255, 1)):
            want[ids == e] = per[k][ids == e]
        for kind in ("dense", "strided", "host"):
            cases.assert_eval(f"256 materials, {kind}", _call(s, ids, i, o, 1, kind), want, np.ones(n, bool))
        djb.set_utia_exact_only(gpu_ctx, True)
        try:
            cases.assert_eval("256 materials, exact only", _call(s, ids, i, o, 1, "dense"), want, np.ones(n, bool))
        finally:
            djb.set_utia_exact_only(gpu_ctx, False)
    finally:
        s.close()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 5. a wave of dead hits, all-dead batches
@pytest.mark.parametrize("n", [64, 300])
def test_all_dead_batches(uset, n):
    _, i, o = cases.grid_block()
    ids = cases.merl_set_cases.inactive_values(cases.M)[np.arange(n) % 5]
    for layout in LAYOUTS:
        for want_cos in (0, 1):
            assert not _call(uset, ids, i[:n], o[:n], want_cos, layout).view(np.uint32).any()


def test_a_wave_of_dead_hits_among_live_ones(uset):
    ids, i, o = (a.copy() for a in cases.grid_block())
    ids[64:128] = -1                                  # one whole wave of the first workgroup
    ids[256 + 192:512] = cases.M                      # the last wave of the second
    want = cases.grid_expected("eval").copy()
    want[~cases.active(ids, cases.M)] = 0
    cases.assert_eval("dead waves", _call(uset, ids, i, o, 0, "dense"), want, np.ones(len(ids), bool))


# ------------------------------------------------------------------ 6. graph capture
def test_calls_replay_from_a_captured_graph(gpu_ctx, uset):
    import torch
    lib = _lib.load()
    gids, gi, go = cases.grid_block()
    n = len(gids)
    ids2, _ = cases.material_ids()
    i2, o2 = cases.eval_inputs()
    ok2 = cases.defined(i2, o2)
    sets = [(gids, gi, go), (ids2[ok2][:n], i2[ok2][:n], o2[ok2][:n])]
    ids, i, o = (resident(gpu_ctx, a) for a in sets[0])
    outs = [torch.zeros((3, n), dtype=torch.float32, device=dev(gpu_ctx)) for _ in range(4)]
    vi, vo = view(i.data_ptr(), n, "dense"), view(o.data_ptr(), n, "dense")
    vouts = [view(a.data_ptr(), n, "dense") for a in outs]

    def launch():                           # four device-memory calls
        for k, vout in enumerate(vouts):
            _lib.check(lib.djb_utia_set_eval_batch(gpu_ctx._h, uset._h, C.c_int64(n), C.c_void_p(ids.data_ptr()), C.byref(vi), C.byref(vo), C.c_int(k & 1),
                                                   C.byref(vout), C.c_int(_lib.MEM_DEVICE)))
    want = graph_replay(gpu_ctx, launch, outs, loads(gpu_ctx, (ids, i, o), sets))
    assert want[0][1].abs().sum() > 0 and not torch.equal(want[0][1], want[1][1])


# ------------------------------------------------------------------ 7. aliasing
@pytest.mark.parametrize("layout", ["dense", "strided"])
def test_in_place_call_equals_out_of_place(gpu_ctx, uset, layout):
    ids, i, o = cases.grid_block()
    n = len(ids)
    want = _call(uset, ids, i, o, 1, layout)
    got = _call(uset, ids, i, o, 1, layout, over="i")      # the output arrays are i's arrays
    cases.assert_eval(f"in place, {layout}", got, want, np.ones(n, bool))
    cases.assert_eval(f"in place, {layout}, against the oracle", got, cases.grid_expected("evalp"), np.ones(n, bool))


def test_output_over_the_ids_equals_out_of_place(gpu_ctx, uset):
    """The ids are an input stream too: the x plane of the output is the id array itself, index-aligned.  Tier 1 declines the block's hits
    and tier 2 would re-read their ids after tier 1 wrote placeholders over them, so the call has to take the exact kernel -- with the
    default worklist, and with a worklist of 0 entries, where tier 2 would redo the whole batch."""
    ids, i, o = cases.grid_block()
    n = len(ids)
    want = _call(uset, ids, i, o, 1, "dense")
    A = Arrays(gpu_ctx, n, "dense")
    vi, vo = A.vec_in(i), A.vec_in(o)
    try:
        for cap in (-1, 0):
            djb.set_test_worklist_cap(gpu_ctx, cap)
            host = np.zeros((n, 3), np.float32)
            host.view(np.int32)[:, 0] = ids                # plane 0: the int32 bits of the ids
            vbuf = A.vec_in(host)
            _lib.check(_lib.load().djb_utia_set_eval_batch(gpu_ctx._h, uset._h, C.c_int64(n), C.c_void_p(vbuf.x), C.byref(vi), C.byref(vo), C.c_int(1),
                                                           C.byref(vbuf), C.c_int(A.mem)))
            got = A.read(vbuf)
            cases.assert_eval(f"output over the ids, cap {cap}", got, want, np.ones(n, bool))
            cases.assert_eval(f"output over the ids, cap {cap}, against the oracle", got, cases.grid_expected("evalp"), np.ones(n, bool))
    finally:
        djb.set_test_worklist_cap(gpu_ctx, -1)


# ------------------------------------------------------------------ 8. contexts
def test_a_set_of_another_context_is_refused(gpu_ctx, uset):
    lib = _lib.load()
    ids, i, o = cases.grid_block()
    other = djb.Context(gpu_ctx.device)
    cpu = djb.cpu_context()
    for ctx, layout, what in ((other, "host", "another context"), (other, "dense", "another context"), (cpu, "host", "different back ends")):
        with pytest.raises(djb.exc) as e:
            _call(uset, ids[:300], i[:300], o[:300], 0, layout, ctx=ctx)
        assert e.value.status == 1 and what in str(e.value), str(e.value)
    foreign = djb.utia.from_table(cases.tables()[1], ctx=other)
    ptrs = (C.c_void_p * 1)(foreign._h.value)
    out = C.c_void_p()
    st = lib.djb_utia_set_create(gpu_ctx._h, C.c_int(1), ptrs, C.byref(out))
    assert st == 1 and "another context" in lib.djb_last_error().decode(errors="replace")
    cases.assert_eval("own context", _call(uset, ids[:300], i[:300], o[:300], 0, "dense"), cases.grid_expected("eval")[:300], np.ones(300, bool))

