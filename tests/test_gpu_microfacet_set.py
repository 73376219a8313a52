"""Microfacet sets on the GPU (djb_kernels_microfacet_set.hip): eval / evalp / pdf, the fused forms, sample and evalp_is of hits on M
resident ggx or beckmann materials against the oracle's per-material results selected by id (tests/microfacet_set_cases.py) -- bits equal in
host, dense and strided layouts and at the sizes where a tile bound can go wrong --, one Fresnel kind against a mixed set, rows in LDS
and rows in global memory, a set just above the LDS budget, DJB_MICROFACET_SET_MAX rows, a second grid-stride trip, dead waves, in-place
calls, graph capture and DJB_OPT_CONTRACT_1E5.

Every output buffer is one unit longer than the batch and the extra unit is checked after the call."""
import ctypes as C

import numpy as np
import pytest

import microfacet_set_cases as cases
from dj_brdf_amd import _lib, djb
from hit_calls import Arrays, dev, graph_replay, loads, resident, view

pytestmark = pytest.mark.gpu
PREFIXES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025)
LAYOUTS = ("host", "dense", "strided")
ROWS_LDS = 200                 # rows: MF_ROWS_LDS of djb_kernels_microfacet_set.hip
GRID_CAP = 256 * 8             # workgroups: GRID_CAP of djb_kernels_microfacet_set.hip (rows in LDS)
# op -> (want bits of djb_microfacet_set_eval_batch, outputs) / (evalp_is?, outputs)
EVAL = {"eval": (1, ("fr",)), "evalp": (2, ("fr",)), "pdf": (4, ("pdf",)), "eval_pdf": (5, ("fr", "pdf")), "evalp_pdf": (6, ("fr", "pdf"))}
SAMPLE = {"sample": (False, ("i",)), "evalp_is": (True, ("w", "i", "pdf"))}
OPS = tuple(EVAL) + tuple(SAMPLE)


@pytest.fixture(scope="module")
def sets(gpu_ctx):
    """the main set of each kind, built from brdf objects that are closed before the first call"""
    out = {}
    for kind in cases.KINDS:
        members, params = cases.product_members(kind, gpu_ctx)
        out[kind] = djb.microfacet_set(members, params, ctx=gpu_ctx)
        for b in members:
            b.close()
        assert out[kind].n_materials == cases.M and out[kind].kind == kind
    yield out
    for s in out.values():
        s.close()


def _call(s, op, ids, a, b, c=None, layout="dense", ctx=None, over={}):
    """one call through the C ABI.  eval ops: a, b = i, o; sampling ops: a, b, c = u1, u2, o.  over = {output: input}: that output's
    arrays are that input's arrays.  -> {output name: array}"""
    ctx = ctx or s.ctx
    n = len(ids)
    A = Arrays(ctx, n, layout)
    mem = C.c_int(A.mem)
    lib = _lib.load()
    pid = A.arr_in(ids, np.int32)

    def out(name, make, wanted):
        if not wanted:
            return None
        if name not in over:
            return make(name)
        return C.byref(ins[over[name]]) if make == A.vec_out else ins[over[name]]
    if op in EVAL:
        want, outs = EVAL[op]
        ins = {"i": A.vec_in(a), "o": A.vec_in(b)}
        _lib.check(lib.djb_microfacet_set_eval_batch(ctx._h, s._h, C.c_int64(n), pid, C.byref(ins["i"]), C.byref(ins["o"]), C.c_int(want),
                                                     out("fr", A.vec_out, "fr" in outs), out("pdf", A.arr_out, "pdf" in outs), mem))
    else:
        is_, outs = SAMPLE[op]
        ins = {"u1": A.arr_in(a), "u2": A.arr_in(b), "o": A.vec_in(c)}
        _lib.check(lib.djb_microfacet_set_sample_batch(ctx._h, s._h, C.c_int64(n), pid, ins["u1"], ins["u2"], C.byref(ins["o"]),
                                                       out("w", A.vec_out, is_), out("i", A.vec_out, True), out("pdf", A.arr_out, is_), mem))
    return dict(A.results(op), **{name: A.read(ins[src]) for name, src in over.items()})


def _inputs(op, ev, sm, n=None):
    """the arguments of _call after ids for op: ev = (i, o), sm = (o, u1, u2)"""
    sl = slice(None, n)
    return (ev[0][sl], ev[1][sl], None) if op in EVAL else (sm[1][sl], sm[2][sl], sm[0][sl])


def _wanted(op, want_eval, want_sample):
    """{output name: array} for op from {eval op: array} and (weight, i, pdf, i of sample)"""
    if op in EVAL:
        fr = want_eval["evalp" if op.startswith("evalp") else "eval"]
        return {k: v for k, v in (("fr", fr), ("pdf", want_eval["pdf"])) if k in EVAL[op][1]}
    return {"i": want_sample[3]} if op == "sample" else dict(zip(("w", "i", "pdf"), want_sample[:3]))


def _check(tag, got, want, n=None):
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for name in got:
        cases.assert_bits(f"{tag}: {name}", got[name], want[name][:n])


def _main_wanted(kind, op):
    return _wanted(op, {o: cases.expected_eval(kind, o) for o in cases.EVAL_OPS}, cases.expected_sample(kind))


def _mix(kind, op):
    """(arguments after ids, wanted outputs) of op on the mixing block"""
    ids, i, o, u1, u2 = cases.mix_block()
    want = cases.mix_expected(kind)
    return _inputs(op, (i, o), (o, u1, u2)), _wanted(op, want, want["evalp_is"] + (want["sample"],))


# ------------------------------------------------------------------ 1. bits equal to the oracle selection: every op x layout x prefix
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("op", OPS)
def test_op_equals_the_oracle_selection(sets, kind, op):
    s = sets[kind]
    ids, bulk = cases.material_ids()
    cases.assert_ids_cover_every_class(ids, bulk, cases.M)
    cases.assert_materials_are_what_the_module_says()
    ev, sm = cases.eval_inputs(), cases.sample_inputs()
    want = _main_wanted(kind, op)
    for layout in LAYOUTS:
        _check(f"{kind} {op}, {layout}, n = {cases.N}", _call(s, op, ids, *_inputs(op, ev, sm), layout=layout), want)
    for n in PREFIXES:                     # units are independent: a prefix has the prefix's results
        for layout in LAYOUTS:
            _check(f"{kind} {op}, {layout}, n = {n}", _call(s, op, ids[:n], *_inputs(op, ev, sm, n), layout=layout), want, n)


# ------------------------------------------------------------------ 2. one wave mixes rows, Fresnel kinds and flags: rows in LDS, rows in global memory, contract mode
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("setting", ["default", "rows global", "contract 1e-5"])
def test_mixing_block(gpu_ctx, sets, kind, setting):
    cases.assert_mix_block_mixes()
    ids = cases.mix_block()[0]
    try:
        if setting == "rows global":
            djb.set_microfacet_set_rows_global(gpu_ctx, True)
        elif setting == "contract 1e-5":
            djb.set_contract_1e5(gpu_ctx, True)
        for op in OPS:
            args, want = _mix(kind, op)
            for layout in ("dense", "strided"):
                got = _call(sets[kind], op, ids, *args, layout=layout)
                _check(f"mixing block, {kind}, {setting}, {op}, {layout}", got, want)
                for a in got.values():
                    assert not a[~cases.active(ids, cases.M)].view(np.uint32).any()
    finally:
        djb.set_microfacet_set_rows_global(gpu_ctx, False)
        djb.set_contract_1e5(gpu_ctx, False)


# ------------------------------------------------------------------ 3. one Fresnel kind (the compile-time route) against a mixed set
@pytest.mark.parametrize("kind", cases.KINDS)
def test_one_fresnel_kind_and_a_mixed_set_give_the_same_bits(gpu_ctx, kind):
    nu = len(cases.UNIFORM)
    uni, mixed = cases.product_set(kind, gpu_ctx, cases.UNIFORM), cases.product_set(kind, gpu_ctx, cases.MIXED)
    try:
        ev, sm = cases.eval_inputs(), cases.sample_inputs()
        ids_m = cases.ids_below(len(cases.MIXED), nu)
        for op in ("evalp_pdf", "eval", "evalp_is"):
            res = {}
            for name, s, ids, mats, limit in (("uniform", uni, cases.material_ids(nu)[0], cases.UNIFORM, None), ("mixed", mixed, ids_m, cases.MIXED, nu)):
                want = _wanted(op, {o: cases.expected_eval(kind, o, mats, limit) for o in cases.EVAL_OPS}, cases.expected_sample(kind, mats, limit))
                for layout in ("dense", "strided"):
                    _check(f"{kind}, {name}, {op}, {layout}", _call(s, op, ids, *_inputs(op, ev, sm), layout=layout), want)
                res[name] = _call(s, op, ids_m, *_inputs(op, ev, sm))                # ... and both on the SAME ids
            for out in res["uniform"]:
                assert cases.same_bits(res["uniform"][out], res["mixed"][out]).all(), (kind, op, out)
    finally:
        uni.close(); mixed.close()


# ------------------------------------------------------------------ 4. just above the LDS budget, and the upper end: rows from global memory
def _cycled(kind, ctx, m):
    mats = [(cases.mk_fresnel(f), sh, cases.mk_params(p)) for f, sh, p in cases.MATERIALS]
    return djb.microfacet_set.from_materials(kind, [mats[k % cases.M] for k in range(m)], ctx=ctx)


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("m", [ROWS_LDS, ROWS_LDS + 1, cases.SET_MAX])
def test_large_sets(gpu_ctx, kind, m):
    at = {0: 0, 1: 1, m // 2: (m // 2) % cases.M, m - 2: (m - 2) % cases.M, m - 1: (m - 1) % cases.M}      # id -> material of the main set, cycled
    assert len(set(at.values())) >= 4
    s = _cycled(kind, gpu_ctx, m)
    try:
        assert s.n_materials == m
        _, i, o, u1, u2 = cases.mix_block()
        n = len(i)
        ids = np.int32([0, 1, m // 2, m - 2, m - 1, m, -1])[np.arange(n) % 7]               # both ends, and the first id outside
        local = np.full(n, -1, np.int32)
        for e, k in at.items():
            local[ids == e] = k
        for op in ("evalp_pdf", "evalp_is", "sample"):
            if op in EVAL:
                per_e = {o_: cases._eval_per(kind, cases.MATERIALS, o_, i, o) for o_ in ("evalp", "pdf")}
                want = {"fr": cases.select(per_e["evalp"], local, cases.M), "pdf": cases.select(per_e["pdf"], local, cases.M)}
            else:
                per = cases._sample_per(kind, cases.MATERIALS, o, u1, u2)
                sel = [cases.select([r[c] for r in per], local, cases.M) for c in range(4)]
                want = _wanted(op, None, sel)
            for layout in LAYOUTS:
                _check(f"{m} rows, {kind}, {op}, {layout}", _call(s, op, ids, *_inputs(op, (i, o), (o, u1, u2)), layout=layout), want)
    finally:
        s.close()


# ------------------------------------------------------------------ 5. a second, ragged grid-stride trip (the grid is capped while the rows are in LDS)
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("op", ["evalp_pdf", "evalp_is"])
def test_second_grid_stride_trip(sets, kind, op):
    """GRID_CAP workgroups cover GRID_CAP * 256 hits; the one hit behind them sends the first workgroup on a second trip"""
    ids = cases.mix_block()[0]
    args, want = _mix(kind, op)
    n = GRID_CAP * 256 + 1
    reps = -(-n // len(ids))
    tile = lambda a: None if a is None else np.ascontiguousarray(np.concatenate([a] * reps)[:n])
    got = _call(sets[kind], op, tile(ids), *[tile(a) for a in args])
    _check(f"second trip, {kind}, {op}", got, {k: tile(v) for k, v in want.items()})


# ------------------------------------------------------------------ 6. waves of dead hits, all-dead batches
@pytest.mark.parametrize("n", [64, 300])
def test_all_dead_batches(sets, n):
    for kind in cases.KINDS:
        ids = cases.inactive_values(cases.M)[np.arange(n) % 5]
        for op in ("eval_pdf", "evalp_is", "sample"):
            args, _ = _mix(kind, op)
            for layout in LAYOUTS:
                for a in _call(sets[kind], op, ids, *[None if x is None else x[:n] for x in args], layout=layout).values():
                    assert not a.view(np.uint32).any()


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("op", ["eval_pdf", "evalp_is"])
def test_the_first_waves_are_wholly_dead(sets, kind, op):
    ids = cases.mix_block()[0].copy()
    ids[:192] = -1                                    # the first three waves of the first workgroup
    ids[256 + 192:512] = cases.M                      # the last wave of the second
    args, want = _mix(kind, op)
    want = {k: v.copy() for k, v in want.items()}
    for v in want.values():
        v[~cases.active(ids, cases.M)] = 0
    for layout in ("dense", "strided"):
        _check(f"dead waves, {kind}, {op}, {layout}", _call(sets[kind], op, ids, *args, layout=layout), want)


# ------------------------------------------------------------------ 7. aliasing
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("layout", ["dense", "strided"])
def test_in_place_calls_equal_out_of_place(gpu_ctx, sets, kind, layout):
    ids, i, o, u1, u2 = cases.mix_block()
    want = cases.mix_expected(kind)
    for which in ("i", "o"):                          # evalp + pdf: fr over i's (o's) arrays
        got = _call(sets[kind], "evalp_pdf", ids, i, o, layout=layout, over={"fr": which})
        cases.assert_bits(f"in place over {which}, {kind}, {layout}", got["fr"], want["evalp"])
        cases.assert_bits(f"in place over {which}, {kind}, {layout}: pdf", got["pdf"], want["pdf"])
    got = _call(sets[kind], "evalp_is", ids, u1, u2, o, layout=layout, over={"i": "o", "pdf": "u1"})      # i over o's arrays, pdf over u1
    for name, out, w in zip(("weight", "i", "pdf"), ("w", "i", "pdf"), want["evalp_is"]):
        cases.assert_bits(f"evalp_is in place, {kind}, {layout}: {name}", got[out], w)


# ------------------------------------------------------------------ 8. graph capture
def test_calls_replay_from_a_captured_graph(gpu_ctx, sets):
    import torch
    lib = _lib.load()
    mids, mi, mo, mu1, mu2 = cases.mix_block()
    n = len(mids)
    ids2, _ = cases.material_ids()
    (i2, o2), (_, u12, u22) = cases.eval_inputs(), cases.sample_inputs()
    data = [(mids, mi, mo, mu1, mu2), (ids2[:n], i2[:n], o2[:n], u12[:n], u22[:n])]
    ids, i, o, u1, u2 = (resident(gpu_ctx, a) for a in data[0])
    vec = lambda: torch.zeros((3, n), dtype=torch.float32, device=dev(gpu_ctx))
    sca = lambda: torch.zeros(n, dtype=torch.float32, device=dev(gpu_ctx))
    outs = {k: {"fr": vec(), "pdf": sca(), "w": vec(), "i": vec(), "ipdf": sca()} for k in cases.KINDS}
    vi, vo = view(i.data_ptr(), n, "dense"), view(o.data_ptr(), n, "dense")

    def launch():                           # two device-memory calls per kind: evalp + pdf, evalp_is
        for k in cases.KINDS:
            a = outs[k]
            _lib.check(lib.djb_microfacet_set_eval_batch(gpu_ctx._h, sets[k]._h, C.c_int64(n), C.c_void_p(ids.data_ptr()), C.byref(vi), C.byref(vo), C.c_int(6),
                                                         C.byref(view(a["fr"].data_ptr(), n, "dense")), C.c_void_p(a["pdf"].data_ptr()), C.c_int(_lib.MEM_DEVICE)))
            _lib.check(lib.djb_microfacet_set_sample_batch(gpu_ctx._h, sets[k]._h, C.c_int64(n), C.c_void_p(ids.data_ptr()), C.c_void_p(u1.data_ptr()),
                                                           C.c_void_p(u2.data_ptr()), C.byref(vo), C.byref(view(a["w"].data_ptr(), n, "dense")),
                                                           C.byref(view(a["i"].data_ptr(), n, "dense")), C.c_void_p(a["ipdf"].data_ptr()), C.c_int(_lib.MEM_DEVICE)))
    want = graph_replay(gpu_ctx, launch, [a for k in cases.KINDS for a in outs[k].values()], loads(gpu_ctx, (ids, i, o, u1, u2), data))
    assert want[0][0].abs().sum() > 0 and not torch.equal(want[0][0], want[1][0])
    cases.assert_bits("eager, ggx evalp", want[0][0].cpu().numpy().T, cases.mix_expected("ggx")["evalp"])


# ------------------------------------------------------------------ 9. set_params in stream order, contexts
def test_set_params_is_seen_by_the_next_call(gpu_ctx):
    ids, i, o, _, _ = cases.mix_block()
    rolled = cases.MATERIALS[1:] + cases.MATERIALS[:1]
    moved = tuple((m[0], m[1], r[2]) for m, r in zip(cases.MATERIALS, rolled))
    s = cases.product_set("ggx", gpu_ctx)
    try:
        _check("before set_params", _call(s, "evalp", ids, i, o), {"fr": cases.mix_expected("ggx")["evalp"]})
        s.set_params([cases.mk_params(m[2]) for m in moved])
        import oraclelib
        O = oraclelib.oracle()
        per = [O.eval(om, i, o, m[2], "evalp") for om, m in zip(cases.oracle_materials("ggx"), moved)]
        _check("after set_params", _call(s, "evalp", ids, i, o), {"fr": cases.select(per, ids, cases.M)})
    finally:
        s.close()


def test_a_set_of_another_context_is_refused(gpu_ctx, sets):
    ids, i, o, _, _ = cases.mix_block()
    other = djb.Context(gpu_ctx.device)
    cpu = djb.cpu_context()
    for ctx, layout, what in ((other, "host", "another context"), (other, "dense", "another context"), (cpu, "host", "different back ends")):
        with pytest.raises(djb.exc) as e:
            _call(sets["ggx"], "eval", ids[:300], i[:300], o[:300], layout=layout, ctx=ctx)
        assert e.value.status == 1 and what in str(e.value), str(e.value)
    foreign = djb.ggx(ctx=other)
    with pytest.raises(djb.exc) as e:
        djb.microfacet_set([foreign], ctx=gpu_ctx)
    assert e.value.status == 1 and "another context" in str(e.value), str(e.value)
