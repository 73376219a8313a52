"""Scenes on the GPU (djb_kernels_scene.hip: the partition by kind and the four per-kind kernels on dense index lists): eval / evalp of hits
that land on a MERL set, a UTIA set, an sgd and an abc model set at once, against the oracle's per-material results selected by scene id
(tests/scene_cases.py) -- bits equal in host, dense and strided layouts, at the sizes where a tile bound can go wrong and across chunk
boundaries --, each kind's second tier inside a mixed batch, scenes with fewer members, dead hits, a later grid-stride trip of every
per-kind kernel, graph capture, in-place calls and the refusals.

Every output buffer is one unit longer than the batch and the extra unit is checked after the call."""
import ctypes as C

import numpy as np
import pytest

import merl_set_cases
import model_set_cases
import scene_cases as cases
import utia_set_cases
from dj_brdf_amd import _lib, djb
from hit_calls import Arrays, dev, graph_replay, loads, resident, view

pytestmark = pytest.mark.gpu
PREFIXES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025)
LAYOUTS = ("host", "dense", "strided")
GRID_CAP = {"merl": 256 * 16, "utia": 256 * 64, "sgd": 256 * 16, "abc": 256 * 16}      # workgroups: the GRID_CAP_* of djb_kernels_scene.hip
KIND_VALUE = {"merl": 3, "utia": 4, "sgd": 6, "abc": 7}


@pytest.fixture(scope="module")
def members(gpu_ctx):
    """the four member sets, built as the set tests build them; their sources are destroyed before the first call"""
    out = {}
    src = merl_set_cases.product_members(gpu_ctx)
    out["merl"] = djb.merl_set(src, ctx=gpu_ctx)
    for b in src:
        b.close()
    src = utia_set_cases.product_members(gpu_ctx)
    out["utia"] = djb.utia_set(src, ctx=gpu_ctx)
    for b in src:
        b.close()
    for kind in model_set_cases.KINDS:
        out[kind] = djb.model_set.from_rows(kind, model_set_cases.rows(kind), ctx=gpu_ctx)
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(scope="module")
def main(gpu_ctx, members):
    s = djb.scene(slots=cases.TABLE, ctx=gpu_ctx, **members)
    assert s.n_slots == cases.N_SLOTS and s.members == (3, 3, 6, 6)
    yield s
    s.close()


def _call(s, ids, i, o, want_cos, layout, ctx=None, over=None):
    """one call through the C ABI -> [n, 3]; over = "i" / "o": the output arrays are that input's arrays"""
    ctx = ctx or s.ctx
    A = Arrays(ctx, len(ids), layout)
    pid, vi, vo = A.arr_in(ids, np.int32), A.vec_in(i), A.vec_in(o)
    alias = {"i": vi, "o": vo}.get(over)
    out = A.vec_out("fr") if alias is None else C.byref(alias)
    _lib.check(_lib.load().djb_scene_eval_batch(ctx._h, s._h, C.c_int64(A.n), pid, C.byref(vi), C.byref(vo), C.c_int(want_cos), out, C.c_int(A.mem)))
    return A.results("eval")["fr"] if alias is None else A.read(alias)


# ------------------------------------------------------------------ 1. bits equal to the oracle selection
@pytest.mark.parametrize("want_cos,op", [(0, "eval"), (1, "evalp")])
def test_eval_equals_the_oracle_selection(main, want_cos, op):
    cases.assert_inputs_are_what_the_module_says()
    ids, _ = cases.material_ids()
    i, o = cases.eval_inputs()
    want = cases.expected(op)
    mask = cases.compared(ids, i, o)
    for layout in LAYOUTS:
        cases.assert_eval(f"{op}, {layout}, n = {cases.N}", _call(main, ids, i, o, want_cos, layout), want, mask)
    for n in PREFIXES:                     # units are independent: a prefix has the prefix's results
        for layout in LAYOUTS:
            cases.assert_eval(f"{op}, {layout}, n = {n}", _call(main, ids[:n], i[:n], o[:n], want_cos, layout), want[:n], mask[:n])
    for per in cases.per_slot(op):
        assert not (cases.same_bits(per, want) | ~mask[:, None]).all()


@pytest.mark.parametrize("want_cos,op", [(0, "eval"), (1, "evalp")])
def test_the_permuted_table(gpu_ctx, members, main, want_cos, op):
    """same members, other slot order, a slot without material and an alias: a result that ignores the table shows"""
    s = djb.scene(slots=cases.TABLE2, ctx=gpu_ctx, **members)
    try:
        ids, _ = cases.material_ids(len(cases.TABLE2))
        i, o = cases.eval_inputs()
        want = cases.expected(op, table=cases.TABLE2)
        mask = cases.compared(ids, i, o, cases.TABLE2)
        for layout in LAYOUTS:
            got = _call(s, ids, i, o, want_cos, layout)
            cases.assert_eval(f"table 2, {op}, {layout}", got, want, mask)
            assert not got[ids == cases.TABLE2.index(None)].view(np.uint32).any()
        other = _call(main, ids, i, o, want_cos, "dense")
        assert not (cases.same_bits(other, want) | ~mask[:, None]).all()
    finally:
        s.close()


@pytest.mark.parametrize("chunk", [1000, 257])
def test_chunk_boundaries(gpu_ctx, main, chunk):
    """the 40 001 hits in chunks of 1 000 and of 257 (a ragged tile in every chunk, a ragged last chunk): the default chunk's bits"""
    ids, _ = cases.material_ids()
    i, o = cases.eval_inputs()
    mask = cases.compared(ids, i, o)
    ref = {op: _call(main, ids, i, o, wc, "dense") for wc, op in ((0, "eval"), (1, "evalp"))}
    try:
        djb.set_test_scene_chunk(gpu_ctx, chunk)
        for wc, op in ((0, "eval"), (1, "evalp")):
            for layout in ("dense", "strided"):
                got = _call(main, ids, i, o, wc, layout)
                cases.assert_eval(f"chunk {chunk}, {op}, {layout}, against the oracle", got, cases.expected(op), mask)
                assert cases.same_bits(got, ref[op]).all(), f"chunk {chunk}, {op}, {layout}: differs from the default chunk"
    finally:
        djb.set_test_scene_chunk(gpu_ctx, 0)


# ------------------------------------------------------------------ 2. each kind's second tier inside a mixed batch
@pytest.mark.parametrize("setting", ["default", "cap 8"])
def test_utia_grid_lines_in_a_mixed_batch(gpu_ctx, main, setting):
    """the pairs tier 1 of the utia kernel declines, interleaved with hits of the other kinds; with a worklist of 8 entries the fix
    kernel redoes the utia segment"""
    ids, i, o, mask = cases.mixed_block("utia")
    try:
        if setting == "cap 8":
            djb.set_test_worklist_cap(gpu_ctx, 8)
        for want_cos, op in ((0, "eval"), (1, "evalp")):
            for layout in ("dense", "strided"):
                cases.assert_eval(f"utia grid lines, {setting}, {op}, {layout}", _call(main, ids, i, o, want_cos, layout), cases.mixed_expected("utia", op), mask)
    finally:
        djb.set_test_worklist_cap(gpu_ctx, -1)


@pytest.mark.parametrize("kind", ["sgd", "abc"])
def test_model_wall_block_in_a_mixed_batch(main, kind):
    ids, i, o, mask = cases.mixed_block(kind)
    for want_cos, op in ((0, "eval"), (1, "evalp")):
        for layout in ("dense", "strided"):
            cases.assert_eval(f"{kind} wall block, {op}, {layout}", _call(main, ids, i, o, want_cos, layout), cases.mixed_expected(kind, op), mask)


@pytest.mark.parametrize("option", ["merl exact only", "utia exact only", "rows global"])
def test_options_of_the_member_sets(gpu_ctx, main, option):
    """merl exact only: every MERL hit goes through the queue; utia exact only: the fix kernel alone over the utia segment; rows global:
    the model kernels read their rows from global memory.  Same bits."""
    setter = {"merl exact only": djb.set_merl_exact_only, "utia exact only": djb.set_utia_exact_only, "rows global": djb.set_model_set_rows_global}[option]
    ids, _ = cases.material_ids()
    i, o = cases.eval_inputs()
    mask = cases.compared(ids, i, o)
    try:
        setter(gpu_ctx, True)
        for want_cos, op in ((0, "eval"), (1, "evalp")):
            for layout in ("dense", "strided"):
                cases.assert_eval(f"{option}, {op}, {layout}", _call(main, ids, i, o, want_cos, layout), cases.expected(op), mask)
        if option == "utia exact only":
            gids, gi, go, gmask = cases.mixed_block("utia")
            cases.assert_eval(f"{option}, grid lines", _call(main, gids, gi, go, 1, "dense"), cases.mixed_expected("utia", "evalp"), gmask)
    finally:
        setter(gpu_ctx, False)


# ------------------------------------------------------------------ 3. scenes with less than the full mix
@pytest.mark.parametrize("kinds", [("merl",), ("utia",), ("sgd",), ("abc",), ("merl", "abc"), ("utia", "sgd"), ("merl", "utia", "sgd"), ("utia", "sgd", "abc")])
def test_scenes_with_fewer_member_sets(gpu_ctx, members, kinds):
    """a kind without a set is not launched: its slots have no material and its hits are +0"""
    absent = [k for k in cases.KINDS if k not in kinds]
    table = cases.table_without(absent)
    s = djb.scene(slots=table, ctx=gpu_ctx, **{k: members[k] for k in kinds})
    try:
        assert s.members == tuple(cases.COUNTS[k] if k in kinds else 0 for k in cases.KINDS)
        ids, _ = cases.material_ids()
        i, o = cases.eval_inputs()
        want = cases.expected("evalp", table=table)
        mask = cases.compared(ids, i, o, table)
        for layout in ("dense", "strided"):
            got = _call(s, ids, i, o, 1, layout)
            cases.assert_eval(f"members {kinds}, {layout}", got, want, mask)
            assert not got[cases.kind_of_ids(ids, table) < 0].view(np.uint32).any()
    finally:
        s.close()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_all_hits_of_one_kind(main, kind):
    """the other three kernels launch, read a count of 0 and leave"""
    i, o = cases.eval_inputs()
    n = 5003
    ids = (cases.base(kind) + np.arange(n) % cases.COUNTS[kind]).astype(np.int32)
    for want_cos, op in ((0, "eval"), (1, "evalp")):
        got = _call(main, ids, i[:n], o[:n], want_cos, "dense")
        cases.assert_eval(f"all {kind}, {op}", got, cases.expected(op, ids, n=n), cases.compared(ids, i[:n], o[:n]))


@pytest.mark.parametrize("n", [1, 64, 300])
def test_all_dead_batches(main, n):
    i, o = cases.eval_inputs()
    ids = merl_set_cases.inactive_values(cases.N_SLOTS)[np.arange(n) % 5]
    for layout in LAYOUTS:
        for want_cos in (0, 1):
            assert not _call(main, ids, i[:n], o[:n], want_cos, layout).view(np.uint32).any()


def test_a_wave_of_dead_hits_among_live_ones(main):
    ids = np.array(cases.material_ids()[0][:4096])
    i, o = (a[:4096] for a in cases.eval_inputs())
    ids[64:128] = -1                                  # one whole wave of the first tile
    ids[512 + 192:512 + 256] = cases.N_SLOTS          # one of the second
    want = cases.expected("eval", ids, n=4096)
    got = _call(main, ids, i, o, 0, "dense")
    cases.assert_eval("dead waves", got, want, cases.compared(ids, i, o))
    assert not got[64:128].view(np.uint32).any() and not got[512 + 192:512 + 256].view(np.uint32).any()


# ------------------------------------------------------------------ 4. a later grid-stride trip of every per-kind kernel
def _trip_case(kind):
    """GRID_CAP * 256 + 4 096 - 179 hits of `kind` behind 300 hits of the main batch: GRID_CAP workgroups cover GRID_CAP * 256 list
    entries, the rest sends sixteen workgroups on a second trip, the last one ragged"""
    n_kind = GRID_CAP[kind] * 256 + 4096 - 179
    head = 300
    mids, mi, mo = cases.material_ids()[0][:head], cases.eval_inputs()[0][:head], cases.eval_inputs()[1][:head]
    if kind == "merl":                                # the main batch's pairs on MERL ids
        bi, bo = cases.eval_inputs()
        bids = (np.arange(len(bi)) % cases.COUNTS["merl"]).astype(np.int32)
        per = merl_set_cases.eval_per_material("evalp")
        bwant = merl_set_cases.select(per, bids)
        bmask = np.ones(len(bids), bool)
    else:
        bids, bi, bo, bmask = cases.mixed_block(kind)
        bwant = cases.mixed_expected(kind, "evalp")
        own = cases.kind_of_ids(bids) == cases.KINDS.index(kind)      # the block's own hits only
        bids, bi, bo, bmask, bwant = bids[own], bi[own], bo[own], bmask[own], bwant[own]
    reps = -(-n_kind // len(bids))
    tile = lambda a, b: np.ascontiguousarray(np.concatenate([a] + [b] * reps)[:head + n_kind])
    ids, i, o = tile(mids, bids), tile(mi, bi), tile(mo, bo)
    want = tile(cases.expected("evalp", n=head), bwant)
    mask = tile(cases.compared(mids, mi, mo), bmask)
    assert (cases.kind_of_ids(ids) == cases.KINDS.index(kind)).sum() >= n_kind - 179
    return ids, i, o, want, mask


@pytest.mark.parametrize("kind", cases.KINDS)
def test_second_grid_stride_trip(gpu_ctx, main, kind):
    ids, i, o, want, mask = _trip_case(kind)
    got = _call(main, ids, i, o, 1, "dense")
    cases.assert_eval(f"second trip, {kind}", got, want, mask)
    if kind == "merl":
        # every MERL hit queued: the ragged last workgroup's waves hold fewer than 64 records when the loop ends -- a residue for the
        # flushing trip whatever tier 1 would have declined
        try:
            djb.set_merl_exact_only(gpu_ctx, True)
            got = _call(main, ids, i, o, 1, "dense")
        finally:
            djb.set_merl_exact_only(gpu_ctx, False)
        cases.assert_eval("second trip, merl, every hit queued", got, want, mask)


# ------------------------------------------------------------------ 5. graph capture
def test_calls_replay_from_a_captured_graph(gpu_ctx, main):
    """after one warm call, four calls -- eval and evalp on two id streams -- captured into one graph and replayed twice with fresh inputs"""
    import torch
    lib = _lib.load()
    n = 8192
    ids_a, i_a, o_a, _ = cases.mixed_block("utia")
    i_b, o_b = (a[:n] for a in cases.eval_inputs())

    def only_defined(ids, i, o):                      # the replays are held against direct calls on every hit: defined values only
        ids = np.array(ids)
        ids[~utia_set_cases.defined(i, o)] = -1
        return ids
    ids_b = cases.material_ids()[0][:n]
    assert cases.mixed_block("utia")[3].all()         # the block itself has no undefined utia hit
    sets = [(ids_a, only_defined(ids_b, i_a, o_a), i_a, o_a), (only_defined(ids_b, i_b, o_b), only_defined(ids_a[::-1], i_b, o_b), i_b, o_b)]
    ids0, ids1, i, o = (resident(gpu_ctx, a) for a in sets[0])
    outs = [torch.zeros((3, n), dtype=torch.float32, device=dev(gpu_ctx)) for _ in range(4)]
    vi, vo = view(i.data_ptr(), n, "dense"), view(o.data_ptr(), n, "dense")
    vouts = [view(a.data_ptr(), n, "dense") for a in outs]

    def launch():                           # four device-memory calls: (ids0, eval), (ids0, evalp), (ids1, eval), (ids1, evalp)
        for k, vout in enumerate(vouts):
            _lib.check(lib.djb_scene_eval_batch(gpu_ctx._h, main._h, C.c_int64(n), C.c_void_p((ids0, ids1)[k >> 1].data_ptr()), C.byref(vi), C.byref(vo),
                                                C.c_int(k & 1), C.byref(vout), C.c_int(_lib.MEM_DEVICE)))
    want = graph_replay(gpu_ctx, launch, outs, loads(gpu_ctx, (ids0, ids1, i, o), sets))
    bits = lambda a: a.view(torch.int32)              # the main batch's pairs hold NaN components: results are compared as bits
    assert want[0][1][:, 0::2].abs().sum() > 0 and not torch.equal(bits(want[0][1]), bits(want[1][1])) and not torch.equal(bits(want[0][1]), bits(want[0][3]))
    cases.assert_eval("direct call before capture", want[0][1].cpu().numpy().T, cases.mixed_expected("utia", "evalp"), cases.mixed_block("utia")[3])


# ------------------------------------------------------------------ 6. aliasing
@pytest.mark.parametrize("layout", ["dense", "strided"])
@pytest.mark.parametrize("over", ["i", "o"])
def test_in_place_call_equals_out_of_place(gpu_ctx, main, layout, over):
    ids, i, o, mask = cases.mixed_block("utia")
    want = _call(main, ids, i, o, 1, layout)
    got = _call(main, ids, i, o, 1, layout, over=over)      # the output arrays are an input's arrays
    assert cases.same_bits(got, want).all(), f"in place over {over}, {layout}: differs from the out-of-place call"
    cases.assert_eval(f"in place over {over}, {layout}, against the oracle", got, cases.mixed_expected("utia", "evalp"), mask)


# ------------------------------------------------------------------ 7. refusals
def _create(ctx, members, slots, n=None):
    lib = _lib.load()
    table = (_lib.SceneSlot * max(len(slots), 1))()
    for k, (kind, local) in enumerate(slots):
        table[k].kind, table[k].local = KIND_VALUE.get(kind, kind), local
    h = C.c_void_p()
    ptr = lambda k: getattr(getattr(members.get(k), "_h", None), "value", None)
    st = lib.djb_scene_create(ctx._h, ptr("merl"), ptr("utia"), ptr("sgd"), ptr("abc"), C.c_int(len(slots) if n is None else n), table, C.byref(h))
    msg = lib.djb_last_error().decode(errors="replace")
    if st == 0:
        lib.djb_scene_destroy(h)
    return st, msg


def test_refusals(gpu_ctx, members, main):
    ids, _ = cases.material_ids()
    i, o = cases.eval_inputs()
    other = djb.Context(gpu_ctx.device)
    cpu = djb.cpu_context()
    for ctx, layout, what in ((other, "host", "another context"), (other, "dense", "another context"), (cpu, "host", "different back ends")):
        with pytest.raises(djb.exc) as e:                                             # a scene of another context
            _call(main, ids[:300], i[:300], o[:300], 0, layout, ctx=ctx)
        assert e.value.status == 1 and what in str(e.value), str(e.value)
    one = [("merl", 0)]
    st, msg = _create(other, members, one)                                            # member sets of another context
    assert st == 1 and "another context" in msg, (st, msg)
    st, msg = _create(gpu_ctx, members, one + [("utia", 3)])                          # local out of range
    assert st == 1 and "slot 1" in msg and "outside" in msg, (st, msg)
    st, msg = _create(gpu_ctx, {"merl": members["merl"]}, one + [("abc", 0)])         # a slot naming an absent set
    assert st == 1 and "slot 1" in msg and "no abc set" in msg, (st, msg)
    for n in (0, cases.SCENE_MAX_SLOTS + 1):
        st, msg = _create(gpu_ctx, members, one, n=n)
        assert st == 1 and "1 .. 1048576" in msg, (st, msg)
    st, msg = _create(gpu_ctx, dict(members, abc=members["sgd"]), one)                # an sgd model set passed as abc
    assert st == 1 and "abc member" in msg, (st, msg)
    st, msg = _create(gpu_ctx, members, one)
    assert st == 0, msg
    cases.assert_eval("own context", _call(main, ids[:300], i[:300], o[:300], 0, "dense"), cases.expected("eval", n=300), cases.compared(ids, i, o)[:300])
    other.close()
