"""The two per-hit proxy steps of a scene on the GPU (djb_kernels_scene_proxy.hip: the partition with its scatter into every output and the
per-kind kernels on dense index lists): the sampling step and the light sample of hits that land on a MERL set, a UTIA set, an sgd and an abc
model set at once, against the oracle's per-slot results selected by scene id (tests/scene_proxy_cases.py) -- bits equal in host, dense and
strided layouts, at the sizes where a tile bound can go wrong and across chunk boundaries --, the second tiers inside a mixed batch, the
member sets' options, scenes with fewer members, dead hits, a later grid-stride trip of every per-kind kernel, graph capture, in-place
calls and the refusals.

Every output buffer is one unit longer than the batch and the extra unit is checked after the call."""
import ctypes as C

import numpy as np
import pytest

import merl_set_cases
import model_set_cases
import scene_proxy_cases as cases
import utia_set_cases
from dj_brdf_amd import _lib, djb
from hit_calls import CANARY, Arrays, dev, graph_replay, loads, resident, view

pytestmark = pytest.mark.gpu
PREFIXES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025)
LAYOUTS = ("host", "dense", "strided")


def _members(ctx, prepared=True):
    """the four member sets, built as the set tests build them; their sources are destroyed before the first call"""
    out = {}
    src = merl_set_cases.product_members(ctx)
    out["merl"] = djb.merl_set(src, ctx=ctx)
    for b in src:
        b.close()
    src = utia_set_cases.product_members(ctx)
    out["utia"] = djb.utia_set(src, ctx=ctx)
    for b in src:
        b.close()
    for kind in model_set_cases.KINDS:
        out[kind] = djb.model_set.from_rows(kind, model_set_cases.rows(kind), ctx=ctx)
    if prepared:
        cases.prepare_members(out)
    return out


@pytest.fixture(scope="module")
def members(gpu_ctx):
    out = _members(gpu_ctx)
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(scope="module")
def main(gpu_ctx, members):
    s = djb.scene(slots=cases.TABLE, ctx=gpu_ctx, **members)
    yield s
    s.close()


@pytest.fixture(scope="module")
def lobes(gpu_ctx):
    return {"ggx": djb.ggx(ctx=gpu_ctx), "beckmann": djb.beckmann(ctx=gpu_ctx)}


def _h(x):
    return x._h if x is not None else None


def _sample(s, proxy, ids, u1, u2, o, layout, ctx=None, in_place=False):
    """one sampling call through the C ABI -> (weight [n, 3], i [n, 3], pdf [n]); in_place: out_i names o's arrays"""
    A = Arrays(ctx or s.ctx, len(ids), layout)
    vo = A.vec_in(o)
    _lib.check(_lib.load().djb_scene_evalp_is_proxy_batch(A.ctx._h, s._h, _h(proxy), C.c_int64(A.n), A.arr_in(ids, np.int32), A.arr_in(u1), A.arr_in(u2),
                                                         C.byref(vo), A.vec_out("weight"), C.byref(vo) if in_place else A.vec_out("i"), A.arr_out("pdf"),
                                                         C.c_int(A.mem)))
    res = A.results("sampling")
    return res["weight"], A.read(vo) if in_place else res["i"], res["pdf"]


def _light(s, proxy, ids, i, o, layout, ctx=None, in_place=False):
    """one light-sample call through the C ABI -> (fr [n, 3], pdf [n]); in_place: out_fr names i's arrays"""
    A = Arrays(ctx or s.ctx, len(ids), layout)
    vi, vo = A.vec_in(i), A.vec_in(o)
    _lib.check(_lib.load().djb_scene_evalp_pdf_proxy_batch(A.ctx._h, s._h, _h(proxy), C.c_int64(A.n), A.arr_in(ids, np.int32), C.byref(vi), C.byref(vo),
                                                          C.byref(vi) if in_place else A.vec_out("fr"), A.arr_out("pdf"), C.c_int(A.mem)))
    res = A.results("light sample")
    return A.read(vi) if in_place else res["fr"], res["pdf"]


def _check_sample(tag, s, lobe, pk, ids, table, o, u1, u2, want, layouts=LAYOUTS):
    mask = cases.compared_sample(ids, table, want[1], o)
    for layout in layouts:
        cases.assert_sample(f"{tag}, sampling, {pk}, {layout}, n = {len(ids)}", _sample(s, lobe, ids, u1, u2, o, layout), want, mask)


def _check_light(tag, s, lobe, pk, ids, table, i, o, want, layouts=LAYOUTS):
    mask = cases.compared_light(ids, table, i, o)
    for layout in layouts:
        cases.assert_light(f"{tag}, light sample, {pk}, {layout}, n = {len(ids)}", _light(s, lobe, ids, i, o, layout), want, mask)


# ------------------------------------------------------------------ 1. bits equal to the oracle selection
@pytest.mark.parametrize("pk", cases.PROXY_KINDS)
def test_sampling_equals_the_oracle_selection(main, lobes, pk):
    cases.assert_input_conditions()
    ids = cases.material_ids()
    o, u1, u2 = cases.sampler_inputs()
    want = cases.expected_sample(pk)
    _check_sample("main", main, lobes[pk], pk, ids, cases.TABLE, o, u1, u2, want)
    for n in PREFIXES:                     # units are independent: a prefix has the prefix's results
        _check_sample("prefix", main, lobes[pk], pk, ids[:n], cases.TABLE, o[:n], u1[:n], u2[:n], cases.head(want, n))


@pytest.mark.parametrize("pk", cases.PROXY_KINDS)
def test_light_sample_equals_the_oracle_selection(main, lobes, pk):
    ids = cases.material_ids()
    i, o = cases.light_inputs()
    want = cases.expected_light(pk)
    _check_light("main", main, lobes[pk], pk, ids, cases.TABLE, i, o, want)
    for n in PREFIXES:
        _check_light("prefix", main, lobes[pk], pk, ids[:n], cases.TABLE, i[:n], o[:n], cases.head(want, n))


def test_the_permuted_table(gpu_ctx, members, main, lobes):
    """same members, other slot order, a slot without material and an alias: a result that ignores the table shows"""
    s = djb.scene(slots=cases.TABLE2, ctx=gpu_ctx, **members)
    try:
        ids = cases.material_ids(len(cases.TABLE2))
        o, u1, u2 = cases.sampler_inputs()
        i, lo = cases.light_inputs()
        want_s, want_l = cases.expected_sample("ggx", cases.TABLE2), cases.expected_light("ggx", cases.TABLE2)
        _check_sample("table 2", s, lobes["ggx"], "ggx", ids, cases.TABLE2, o, u1, u2, want_s)
        _check_light("table 2", s, lobes["ggx"], "ggx", ids, cases.TABLE2, i, lo, want_l)
        none = ids == cases.TABLE2.index(None)
        assert not any(a[none].view(np.uint32).any() for a in _sample(s, lobes["ggx"], ids, u1, u2, o, "dense") + _light(s, lobes["ggx"], ids, i, lo, "dense"))
        assert cases.differs(_sample(main, lobes["ggx"], ids, u1, u2, o, "dense"), want_s, cases.compared_sample(ids, cases.TABLE2, want_s[1], o))
        assert cases.differs(_light(main, lobes["ggx"], ids, i, lo, "dense"), want_l, cases.compared_light(ids, cases.TABLE2, i, lo))
    finally:
        s.close()


@pytest.mark.parametrize("chunk", [1000, 257])
def test_chunk_boundaries(gpu_ctx, main, lobes, chunk):
    """the 40 001 hits in chunks of 1 000 and of 257 (a ragged tile in every chunk, a ragged last chunk): the oracle's values, and the
    default chunk's bits on every hit"""
    ids = cases.material_ids()
    o, u1, u2 = cases.sampler_inputs()
    i, lo = cases.light_inputs()
    pk = "beckmann"
    ref_s, ref_l = _sample(main, lobes[pk], ids, u1, u2, o, "dense"), _light(main, lobes[pk], ids, i, lo, "dense")
    try:
        djb.set_test_scene_chunk(gpu_ctx, chunk)
        _check_sample(f"chunk {chunk}", main, lobes[pk], pk, ids, cases.TABLE, o, u1, u2, cases.expected_sample(pk), ("dense", "strided"))
        _check_light(f"chunk {chunk}", main, lobes[pk], pk, ids, cases.TABLE, i, lo, cases.expected_light(pk), ("dense", "strided"))
        for layout in ("dense", "strided"):
            for got, ref in zip(_sample(main, lobes[pk], ids, u1, u2, o, layout) + _light(main, lobes[pk], ids, i, lo, layout), ref_s + ref_l):
                assert cases.same_bits(got, ref).all(), f"chunk {chunk}, {layout}: differs from the default chunk"
    finally:
        djb.set_test_scene_chunk(gpu_ctx, 0)


# ------------------------------------------------------------------ 2. second tiers inside a mixed batch, and the member sets' options
@pytest.mark.parametrize("kind", ["merl", "sgd", "abc"])
def test_second_tier_blocks_in_a_mixed_batch(main, lobes, kind):
    """merl: the pairs tier 1 of the MERL index declines (merl_set_light_cases.declined_block) -- queued and drained among hits of other
    kinds; sgd / abc: the wall block, where the decided tier of the models declines"""
    for pk in cases.PROXY_KINDS:
        ids, i, o = cases.mixed_light(kind)
        _check_light(f"{kind} block", main, lobes[pk], pk, ids, cases.TABLE, i, o, cases.mixed_light_expected(pk, kind), ("dense", "strided"))
        ids, o, u1, u2 = cases.mixed_sample(kind)
        _check_sample(f"{kind} block", main, lobes[pk], pk, ids, cases.TABLE, o, u1, u2, cases.mixed_sample_expected(pk, kind), ("dense", "strided"))


@pytest.mark.parametrize("option", ["merl exact only", "rows global"])
def test_options_of_the_member_sets(gpu_ctx, main, lobes, option):
    """merl exact only: every MERL hit above the guards goes through the queue; rows global: the model kernels read their rows from global
    memory.  Same bits."""
    setter = {"merl exact only": djb.set_merl_exact_only, "rows global": djb.set_model_set_rows_global}[option]
    ids = cases.material_ids()
    o, u1, u2 = cases.sampler_inputs()
    i, lo = cases.light_inputs()
    try:
        setter(gpu_ctx, True)
        for pk in cases.PROXY_KINDS:
            _check_sample(option, main, lobes[pk], pk, ids, cases.TABLE, o, u1, u2, cases.expected_sample(pk), ("dense", "strided"))
            _check_light(option, main, lobes[pk], pk, ids, cases.TABLE, i, lo, cases.expected_light(pk), ("dense", "strided"))
    finally:
        setter(gpu_ctx, False)


# ------------------------------------------------------------------ 3. scenes with less than the full mix
@pytest.mark.parametrize("kinds", [("merl",), ("utia",), ("sgd",), ("abc",), ("sgd", "abc"), ("merl", "abc"), ("utia", "sgd"), ("merl", "utia", "sgd"),
                                   ("utia", "sgd", "abc")])
def test_scenes_with_fewer_member_sets(gpu_ctx, members, lobes, kinds):
    """a kind without a set is not launched: its slots have no material and its hits are +0; model members alone take no lobe"""
    table = cases.table_without([k for k in cases.KINDS if k not in kinds])
    s = djb.scene(slots=table, ctx=gpu_ctx, **{k: members[k] for k in kinds})
    try:
        n = 8001
        ids = cases.material_ids()[:n]
        o, u1, u2 = cases.head(cases.sampler_inputs(), n)
        i, lo = cases.head(cases.light_inputs(), n)
        pk = "ggx"
        lobe = None if set(kinds) <= {"sgd", "abc"} else lobes[pk]
        _check_sample(f"members {kinds}", s, lobe, pk, ids, table, o, u1, u2, cases.expected_sample_on(pk, ids, table, o, u1, u2), ("dense", "strided"))
        _check_light(f"members {kinds}", s, lobe, pk, ids, table, i, lo, cases.expected_light_on(pk, ids, table, i, lo), ("dense", "strided"))
        dead = cases.kind_of_ids(ids, table) < 0
        assert dead.sum() > n // 8 and not any(a[dead].view(np.uint32).any() for a in _sample(s, lobe, ids, u1, u2, o, "dense"))
    finally:
        s.close()


def _one_kind(kind, n):
    """the first n hits of the main inputs, all on materials of `kind`"""
    return (cases.base(kind) + np.arange(n) % cases.COUNTS[kind]).astype(np.int32)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_all_hits_of_one_kind(main, lobes, kind):
    """the other three kernels launch, read a count of 0 and leave"""
    n = 5003
    ids = _one_kind(kind, n)
    o, u1, u2 = cases.head(cases.sampler_inputs(), n)
    i, lo = cases.head(cases.light_inputs(), n)
    for pk in cases.PROXY_KINDS:
        _check_sample(f"all {kind}", main, lobes[pk], pk, ids, cases.TABLE, o, u1, u2, cases.expected_sample_on(pk, ids, cases.TABLE, o, u1, u2), ("dense",))
        _check_light(f"all {kind}", main, lobes[pk], pk, ids, cases.TABLE, i, lo, cases.expected_light_on(pk, ids, cases.TABLE, i, lo), ("dense",))


@pytest.mark.parametrize("n", [1, 64, 300])
def test_all_dead_batches(main, lobes, n):
    o, u1, u2 = cases.head(cases.sampler_inputs(), n)
    i, lo = cases.head(cases.light_inputs(), n)
    ids = merl_set_cases.inactive_values(cases.N_SLOTS)[np.arange(n) % 5]
    for layout in LAYOUTS:
        for a in _sample(main, lobes["ggx"], ids, u1, u2, o, layout) + _light(main, lobes["ggx"], ids, i, lo, layout):
            assert not a.view(np.uint32).any(), (layout, n)


def test_a_wave_of_dead_hits_among_live_ones(main, lobes):
    n = 4096
    ids = np.array(cases.material_ids()[:n])
    ids[64:128] = -1                                  # one whole wave of the first tile
    ids[512 + 192:512 + 256] = cases.N_SLOTS          # one of the second
    o, u1, u2 = cases.head(cases.sampler_inputs(), n)
    i, lo = cases.head(cases.light_inputs(), n)
    _check_sample("dead waves", main, lobes["ggx"], "ggx", ids, cases.TABLE, o, u1, u2, cases.expected_sample_on("ggx", ids, cases.TABLE, o, u1, u2), ("dense",))
    _check_light("dead waves", main, lobes["ggx"], "ggx", ids, cases.TABLE, i, lo, cases.expected_light_on("ggx", ids, cases.TABLE, i, lo), ("dense",))
    for a in _sample(main, lobes["ggx"], ids, u1, u2, o, "dense") + _light(main, lobes["ggx"], ids, i, lo, "dense"):
        assert not a[64:128].view(np.uint32).any() and not a[512 + 192:512 + 256].view(np.uint32).any()


# ------------------------------------------------------------------ 4. a later grid-stride trip of every per-kind kernel
HEAD, TRIP_BLOCK = 300, 4096


def _trip(kind, arrays, expected_on):
    """TRIP_N = GRID_CAP * 256 + 4 096 - 179 hits of `kind` behind 300 hits of the main batch: GRID_CAP workgroups cover GRID_CAP * 256
    list entries, the rest sends sixteen workgroups on a second trip, the last one ragged.  The hits of `kind`: a block of 4 096 hits of
    the main inputs on the kind's materials, tiled; its expectation is computed once and tiled with it"""
    n = HEAD + cases.TRIP_N
    bids = _one_kind(kind, TRIP_BLOCK)
    block = tuple(a[HEAD:HEAD + TRIP_BLOCK] for a in arrays)
    hids = cases.material_ids()[:HEAD]
    heads = cases.head(arrays, HEAD)
    want = cases.tiled(expected_on(hids, *heads), expected_on(bids, *block), n)
    ids, = cases.tiled((hids,), (bids,), n)
    assert (cases.kind_of_ids(ids) == cases.KINDS.index(kind)).sum() >= cases.TRIP_N
    return (ids,) + cases.tiled(heads, block, n), want


@pytest.mark.parametrize("kind", cases.KINDS)
def test_second_grid_stride_trip_of_sampling(gpu_ctx, main, lobes, kind):
    pk = "beckmann"
    (ids, o, u1, u2), want = _trip(kind, cases.sampler_inputs(), lambda ids, o, u1, u2: cases.expected_sample_on(pk, ids, cases.TABLE, o, u1, u2))
    _check_sample(f"second trip, {kind}", main, lobes[pk], pk, ids, cases.TABLE, o, u1, u2, want, ("dense",))
    if kind == "merl":
        # every MERL hit queued: the ragged last workgroup's waves hold fewer than 64 records when the loop ends -- a residue for the
        # flushing trip whatever tier 1 would have declined
        try:
            djb.set_merl_exact_only(gpu_ctx, True)
            _check_sample("second trip, merl, every hit queued", main, lobes[pk], pk, ids, cases.TABLE, o, u1, u2, want, ("dense",))
        finally:
            djb.set_merl_exact_only(gpu_ctx, False)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_second_grid_stride_trip_of_the_light_sample(gpu_ctx, main, lobes, kind):
    pk = "beckmann"
    (ids, i, o), want = _trip(kind, cases.light_inputs(), lambda ids, i, o: cases.expected_light_on(pk, ids, cases.TABLE, i, o))
    _check_light(f"second trip, {kind}", main, lobes[pk], pk, ids, cases.TABLE, i, o, want, ("dense",))
    if kind == "merl":
        try:
            djb.set_merl_exact_only(gpu_ctx, True)
            _check_light("second trip, merl, every hit queued", main, lobes[pk], pk, ids, cases.TABLE, i, o, want, ("dense",))
        finally:
            djb.set_merl_exact_only(gpu_ctx, False)


# ------------------------------------------------------------------ 5. graph capture
def test_calls_replay_from_a_captured_graph(gpu_ctx, main, lobes):
    """after one warm call, four calls -- sampling and the light sample on two id streams -- captured into one graph and replayed twice with
    fresh inputs; the replays are held, as bits, against direct calls"""
    import torch
    lib = _lib.load()
    n = 8192
    lobe = lobes["ggx"]
    so, su1, su2 = cases.sampler_inputs()
    li, lo = cases.light_inputs()
    all_ids = cases.material_ids()

    def data(lo_, ids_a, ids_b):
        sl = slice(lo_, lo_ + n)
        return (np.array(ids_a), np.array(ids_b), su1[sl], su2[sl], so[sl], li[sl], lo[sl])
    sets = [data(0, all_ids[:n], all_ids[n:2 * n][::-1]), data(n, cases.mixed_light("merl")[0], all_ids[2 * n:3 * n])]
    ids0, ids1, u1, u2, o, i, o2 = (resident(gpu_ctx, a) for a in sets[0])
    vec = lambda: torch.zeros((3, n), dtype=torch.float32, device=dev(gpu_ctx))
    sca = lambda: torch.zeros((n,), dtype=torch.float32, device=dev(gpu_ctx))
    outs = [[vec(), vec(), sca(), vec(), sca()] for _ in range(2)]        # per id stream: weight, i, pdf; fr, pdf
    dense = lambda t: view(t.data_ptr(), n, "dense")
    vo, vi, vo2 = dense(o), dense(i), dense(o2)

    def launch():
        for ids, (w, si, pdf, fr, lpdf) in zip((ids0, ids1), outs):
            _lib.check(lib.djb_scene_evalp_is_proxy_batch(gpu_ctx._h, main._h, lobe._h, C.c_int64(n), C.c_void_p(ids.data_ptr()), C.c_void_p(u1.data_ptr()),
                                                          C.c_void_p(u2.data_ptr()), C.byref(vo), C.byref(dense(w)), C.byref(dense(si)),
                                                          C.c_void_p(pdf.data_ptr()), C.c_int(_lib.MEM_DEVICE)))
            _lib.check(lib.djb_scene_evalp_pdf_proxy_batch(gpu_ctx._h, main._h, lobe._h, C.c_int64(n), C.c_void_p(ids.data_ptr()), C.byref(vi), C.byref(vo2),
                                                           C.byref(dense(fr)), C.c_void_p(lpdf.data_ptr()), C.c_int(_lib.MEM_DEVICE)))
    want = graph_replay(gpu_ctx, launch, [a for per in outs for a in per], loads(gpu_ctx, (ids0, ids1, u1, u2, o, i, o2), sets))
    bits = lambda a: a.view(torch.int32)
    assert not torch.equal(bits(want[0][0]), bits(want[1][0])) and not torch.equal(bits(want[0][0]), bits(want[0][5]))
    # the direct calls themselves, against the oracle
    ids_a, ids_b = sets[0][0], sets[0][1]
    got = tuple(a.cpu().numpy().T if a.ndim == 2 else a.cpu().numpy() for a in want[0])
    exp = cases.expected_sample_on("ggx", ids_a, cases.TABLE, so[:n], su1[:n], su2[:n])
    cases.assert_sample("direct call before capture, sampling", got[0:3], exp, cases.compared_sample(ids_a, cases.TABLE, exp[1], so[:n]))
    cases.assert_light("direct call before capture, light sample", got[8:10], cases.expected_light_on("ggx", ids_b, cases.TABLE, li[:n], lo[:n]),
                       cases.compared_light(ids_b, cases.TABLE, li[:n], lo[:n]))


# ------------------------------------------------------------------ 6. aliasing
@pytest.mark.parametrize("layout", ["dense", "strided"])
def test_in_place_calls_equal_out_of_place(gpu_ctx, main, lobes, layout):
    """index-aligned in-place views: out_i over o (sampling) and out_fr over i (the light sample)"""
    lobe = lobes["beckmann"]
    ids, o, u1, u2 = cases.mixed_sample("merl")
    want = _sample(main, lobe, ids, u1, u2, o, layout)
    got = _sample(main, lobe, ids, u1, u2, o, layout, in_place=True)
    for name, g, e in zip(("weight", "i", "pdf"), got, want):
        assert cases.same_bits(g, e).all(), f"sampling in place, {layout}: {name} differs from the out-of-place call"
    exp = cases.mixed_sample_expected("beckmann", "merl")
    cases.assert_sample(f"sampling in place, {layout}, against the oracle", got, exp, cases.compared_sample(ids, cases.TABLE, exp[1], o))

    ids, i, o = cases.mixed_light("merl")
    want = _light(main, lobe, ids, i, o, layout)
    got = _light(main, lobe, ids, i, o, layout, in_place=True)
    for name, g, e in zip(("fr", "pdf"), got, want):
        assert cases.same_bits(g, e).all(), f"light sample in place, {layout}: {name} differs from the out-of-place call"
    cases.assert_light(f"light sample in place, {layout}, against the oracle", got, cases.mixed_light_expected("beckmann", "merl"),
                       cases.compared_light(ids, cases.TABLE, i, o))


# ------------------------------------------------------------------ 7. refusals
def test_refusals(gpu_ctx, main, members, lobes):
    other = djb.Context(gpu_ctx.device)
    other_lobe = djb.ggx(ctx=other)
    try:
        cases.assert_refusals(gpu_ctx, main, members, lobes, other, other_lobe, _members)
        cpu = djb.cpu_context()
        for call in (cases.c_sample, cases.c_light):                                   # a scene of the other back end
            st, msg, outs = call(cpu, main, lobes["ggx"])
            assert st == cases.INVALID and "different back ends" in msg and all((a == CANARY).all() for a in outs), (st, msg)
    finally:
        other_lobe.close(); other.close()
