"""The host staging of the single-material entries (djb_host_ops.hip), at the smallest shapes at which it can go wrong: every operator
body through the chunked host pipeline in three chunks of 2049, 2049 and 1 units (the third reuses slot 0, the tail is one unit) and in
two full chunks, AoS and SoA, against the same call unchunked and against the device-resident call, bit for bit; the pipeline's two
refusals; and the status and message of a large host batch with one array missing, per body and per array."""
import ctypes as C
import os

import numpy as np
import pytest

import proxy_is_cases as cases
from dj_brdf_amd import _lib, djb, synth
from golden_cases import LEAN_BASE, LEAN_SCALE
from test_gpu_parity import mk_params

pytestmark = pytest.mark.gpu
N_TAIL, N_FULL, CHUNK = 4099, 4098, 2049     # SMALL_N = 4096: the smallest batch above it; 2 * CHUNK + 1 and 2 * CHUNK
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INVALID = 1                                   # DJB_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------ one C call described by its arguments
# An argument is a ctypes value passed as it is, the markers N / MEM, or one array of the call:
#   ("iv", name) input vec3 view | ("if", name, width) input floats | ("ov", name) output view | ("of", name, width) output floats
N, MEM = "n", "mem"


def paged(shape, fill=None):
    """a buffer that owns its host pages (test_gpu_parity.py): the chunked path is taken only when inputs and outputs share none"""
    count = int(np.prod(shape))
    raw = np.empty(count + 3072, np.float32)
    off = (-raw.ctypes.data % 4096) // 4
    a = raw[off:off + count].reshape(shape)
    assert a.ctypes.data % 4096 == 0
    a[...] = np.nan if fill is None else fill
    return a


def vec_view(base, n, aos, stride=None):
    v = _lib.Vec3View()
    if aos: v.x, v.y, v.z, v.stride = base, base + 4, base + 8, stride or 3
    else: v.x, v.y, v.z, v.stride = base, base + 4 * n, base + 8 * n, 1
    return v


def call(fn, args, data, n, aos=True, device=False, null=(), place=None):
    """fn(*args) on the first n units of `data` -> (status, message, {output name: array as [n, 3] / [n] / [n, width]}).
    null: names of arrays passed as NULL.  place: {name: (buffer, pointer, vec3 stride)} for arrays the caller laid out itself."""
    import torch
    lib = _lib.load()
    keep, outs, cargs = [], {}, []
    dev = f"cuda:{data['ctx'].device}"

    def buffer(shape, src):
        if device:
            t = torch.full(shape, float("nan"), dtype=torch.float32, device=dev) if src is None else \
                torch.from_numpy(np.ascontiguousarray(src, np.float32).reshape(shape)).to(dev)
            return t, t.data_ptr()
        a = paged(shape, src)
        return a, a.ctypes.data

    for a in args:
        if a is N: cargs.append(C.c_int64(n)); continue
        if a is MEM: cargs.append(C.c_int(_lib.MEM_DEVICE if device else _lib.MEM_HOST)); continue
        if not isinstance(a, tuple): cargs.append(a); continue
        kind, name = a[0], a[1]
        if name in null: cargs.append(None); continue
        src = None if kind[0] == "o" else data[name][:n]
        if kind[1] == "v":
            if place and name in place:
                buf, ptr, stride = place[name]
                v = vec_view(ptr, n, True, stride)
            else:
                dense = aos or device
                buf, ptr = buffer((n, 3) if dense else (3, n), src if src is None or dense else src.T)
                v = vec_view(ptr, n, dense)
            keep.append(v)
            cargs.append(C.byref(v))
            if kind[0] == "o": outs[name] = (buf, "v" if buf.shape[0] == n else "vt")
        else:
            buf, ptr = buffer((n,) if a[2] == 1 else (n, a[2]), src)
            cargs.append(C.c_void_p(ptr))
            if kind[0] == "o": outs[name] = (buf, "f")
        keep.append(buf)
    if device: torch.cuda.synchronize()
    st = fn(*cargs)
    msg = lib.djb_last_error().decode(errors="replace") if st else ""
    if device: torch.cuda.synchronize()
    res = {}
    for name, (buf, how) in outs.items():
        a = buf.cpu().numpy() if device else buf
        res[name] = np.array(a.T if how == "vt" else a[:, :3] if how == "v" else a)
    return st, msg, res


def pipe_env(monkeypatch, chunk, require):
    monkeypatch.setenv("DJB_HOST_PIPE_CHUNK", str(chunk))
    if require: monkeypatch.setenv("DJB_HOST_PIPE_REQUIRE", "1")
    else: monkeypatch.delenv("DJB_HOST_PIPE_REQUIRE", raising=False)


def same_on_every_path(monkeypatch, tag, fn, args, data):
    """unchunked host call == device-resident call == chunked host call in both layouts, at both sizes"""
    for n in (N_TAIL, N_FULL):
        pipe_env(monkeypatch, 0, False)
        st, msg, want = call(fn, args, data, n)
        assert st == 0, (tag, n, msg)
        assert want and all(np.isfinite(v).all() for v in want.values()), (tag, n, "the expected arrays are not all finite")
        st, msg, got = call(fn, args, data, n, device=True)
        assert st == 0, (tag, n, "device", msg)
        for k in want:
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (tag, n, "device", k)
        pipe_env(monkeypatch, CHUNK, True)          # falling back to the plain path is an error here
        for aos in (True, False):
            st, msg, got = call(fn, args, data, n, aos=aos)
            assert st == 0, (tag, n, "chunked", aos, msg)
            for k in want:
                assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (tag, n, "chunked", aos, k)


# ------------------------------------------------------------------ the objects and inputs, built once
@pytest.fixture(scope="module")
def data(gpu_ctx):
    n = N_TAIL
    g = np.load(os.path.join(G, "lean.npz"))
    reps = -(-n // len(g["i"]))
    d = {"ctx": gpu_ctx,
         "i": synth.directions_aos(n, synth.SEED_I), "o": synth.directions_aos(n, synth.SEED_O),
         "u1": synth.uniforms(n, synth.SEED_U1), "u2": synth.uniforms(n, synth.SEED_U2),
         "li": np.tile(g["i"], (reps, 1))[:n], "lo": np.tile(g["o"], (reps, 1))[:n], "lean": np.tile(g["lean"], (reps, 1))[:n],
         "lu1": np.tile(g["u1"], reps)[:n], "lu2": np.tile(g["u2"], reps)[:n]}
    fres = djb.fresnel.schlick((1.0, 0.71, 0.29))
    d["ggx"], d["beckmann"] = djb.ggx(fres, True, ctx=gpu_ctx), djb.beckmann(fres, True, ctx=gpu_ctx)
    d["merl"] = djb.merl.from_table(synth.merl_table_hashed(), ctx=gpu_ctx)
    d["abc"] = cases.product_target("abc", gpu_ctx)
    d["p_ggx"], d["p_beckmann"] = cases.product_proxy("ggx_iso", gpu_ctx), cases.product_proxy("beckmann_ell", gpu_ctx)
    d["iso"], d["ell"], d["base"] = djb.microfacet.params.isotropic(0.3), djb.microfacet.params.elliptic(0.2, 0.5, 0.7), mk_params(LEAN_BASE)
    # the records of the _pp calls: what eval_lean resolves for the LEAN hits (unchunked, below)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("DJB_HOST_PIPE_CHUNK", "0")
        d["pp"] = d["beckmann"].eval_lean(d["li"], d["lo"], d["base"], LEAN_SCALE, d["lean"], want="pdf", return_params=True)[1]
    assert np.isfinite(d["pp"]).all()
    return d


def h(obj):
    return obj._h


def par(p):
    return djb._params_ptr(p)


def eval_calls(d, b, params):
    """eval / evalp / pdf / eval_pdf: want 1, 2, 4, 5 and 6"""
    lib = _lib.load()
    head = [h(d["ctx"]), h(b), N, ("iv", "i"), ("iv", "o"), par(params)]
    return [("eval", lib.djb_eval_batch, head + [("ov", "fr"), MEM]),
            ("evalp", lib.djb_evalp_batch, head + [("ov", "fr"), MEM]),
            ("pdf", lib.djb_pdf_batch, head + [("of", "pdf", 1), MEM]),
            ("eval+pdf", lib.djb_eval_pdf_batch, head + [C.c_int(0), ("ov", "fr"), ("of", "pdf", 1), MEM]),
            ("evalp+pdf", lib.djb_eval_pdf_batch, head + [C.c_int(1), ("ov", "fr"), ("of", "pdf", 1), MEM])]


def sample_calls(d, b, params):
    lib = _lib.load()
    head = [h(d["ctx"]), h(b), N, ("if", "u1", 1), ("if", "u2", 1), ("iv", "o"), par(params)]
    return [("sample", lib.djb_sample_batch, head + [("ov", "i_out"), MEM]),
            ("evalp_is", lib.djb_evalp_is_batch, head + [("ov", "w"), ("ov", "i_out"), ("of", "pdf", 1), MEM])]


def proxy_calls(d, target, proxy, params):
    lib = _lib.load()
    head = [h(d["ctx"]), h(target), h(proxy), N]
    return [("evalp_is_proxy", lib.djb_evalp_is_proxy_batch, head + [("if", "u1", 1), ("if", "u2", 1), ("iv", "o"), None, par(params),
                                                                     ("ov", "w"), ("ov", "i_out"), ("of", "pdf", 1), MEM]),
            ("evalp_pdf_proxy", lib.djb_evalp_pdf_proxy_batch, head + [("iv", "i"), ("iv", "o"), None, par(params),
                                                                       ("ov", "fr"), ("of", "pdf", 1), MEM])]


def eval_pp_call(d, b, want):
    outs = ([("ov", "fr")] if want & 3 else [None]) + ([("of", "pdf", 1)] if want & 4 else [None])
    return (f"eval_pp/{want}", _lib.load().djb_eval_pp_batch,
            [h(d["ctx"]), h(b), N, ("iv", "li"), ("iv", "lo"), ("if", "pp", 5), C.c_int(want)] + outs + [MEM])


def eval_lean_call(d, b, want, params_out=True):
    outs = ([("ov", "fr")] if want & 3 else [None]) + ([("of", "pdf", 1)] if want & 4 else [None])
    return (f"eval_lean/{want}", _lib.load().djb_eval_lean_batch,
            [h(d["ctx"]), h(b), N, ("iv", "li"), ("iv", "lo"), par(d["base"]), C.c_float(LEAN_SCALE), C.c_int(0), ("if", "lean", 5),
             C.c_int(want)] + outs + [("of", "pp_out", 5) if params_out else None, MEM])


def sample_pp_call(d, b, is_):
    outs = [("ov", "w"), ("ov", "i_out"), ("of", "pdf", 1)] if is_ else [None, ("ov", "i_out"), None]
    return (f"sample_pp/{'is' if is_ else 'sample'}", _lib.load().djb_sample_pp_batch,
            [h(d["ctx"]), h(b), N, ("if", "lu1", 1), ("if", "lu2", 1), ("iv", "lo"), ("if", "pp", 5)] + outs + [MEM])


def sample_lean_call(d, b, is_, params_out):
    outs = [("ov", "w"), ("ov", "i_out"), ("of", "pdf", 1)] if is_ else [None, ("ov", "i_out"), None]
    return (f"sample_lean/{'is' if is_ else 'sample'}{'+params' if params_out else ''}", _lib.load().djb_sample_lean_batch,
            [h(d["ctx"]), h(b), N, ("if", "lu1", 1), ("if", "lu2", 1), ("iv", "lo"), par(d["base"]), C.c_float(LEAN_SCALE), C.c_int(0),
             ("if", "lean", 5)] + outs + [("of", "pp_out", 5) if params_out else None, MEM])


# ------------------------------------------------------------------ 1. every body through the chunked path
@pytest.mark.parametrize("kind", ["ggx", "merl"])
def test_eval_bodies_chunked(data, monkeypatch, kind):
    for tag, fn, args in eval_calls(data, data[kind], data["iso"] if kind == "ggx" else None):
        same_on_every_path(monkeypatch, f"{kind}/{tag}", fn, args, data)


@pytest.mark.parametrize("kind", ["ggx", "beckmann"])
def test_sample_bodies_chunked(data, monkeypatch, kind):
    for tag, fn, args in sample_calls(data, data[kind], data["ell"]):
        same_on_every_path(monkeypatch, f"{kind}/{tag}", fn, args, data)


@pytest.mark.parametrize("target,proxy,params", [("merl", "p_ggx", "iso"), ("abc", "p_beckmann", "ell")])
def test_proxy_bodies_chunked(data, monkeypatch, target, proxy, params):
    for tag, fn, args in proxy_calls(data, data[target], data[proxy], data[params]):
        same_on_every_path(monkeypatch, f"{target} <- {proxy}/{tag}", fn, args, data)


def test_eval_pp_and_eval_lean_chunked(data, monkeypatch):
    b = data["beckmann"]
    for tag, fn, args in [eval_pp_call(data, b, 2), eval_pp_call(data, b, 4), eval_pp_call(data, b, 5),
                          eval_lean_call(data, b, 6), eval_lean_call(data, b, 4), eval_lean_call(data, b, 1, params_out=False)]:
        same_on_every_path(monkeypatch, tag, fn, args, data)


@pytest.mark.parametrize("kind", ["ggx", "beckmann"])
def test_sample_pp_and_sample_lean_chunked(data, monkeypatch, kind):
    b = data[kind]
    for tag, fn, args in [sample_pp_call(data, b, False), sample_pp_call(data, b, True)] + \
                         [sample_lean_call(data, b, is_, pp) for is_ in (False, True) for pp in (False, True)]:
        same_on_every_path(monkeypatch, f"{kind}/{tag}", fn, args, data)


def test_chunked_lean_params_are_the_records_of_the_pp_calls(data, monkeypatch):
    """eval_lean and sample_lean return the same resolved records, chunked, and those are what the _pp calls were given"""
    pipe_env(monkeypatch, CHUNK, True)
    for tag, fn, args in (eval_lean_call(data, data["beckmann"], 4), sample_lean_call(data, data["beckmann"], False, True)):
        st, msg, got = call(fn, args, data, N_TAIL)
        assert st == 0, (tag, msg)
        assert np.array_equal(got["pp_out"].view(np.uint32), data["pp"].view(np.uint32)), tag


# ------------------------------------------------------------------ 2. the two refusals of the pipeline
def test_an_output_in_an_input_page_is_refused(data, monkeypatch):
    n = N_TAIL
    tag, fn, args = eval_calls(data, data["ggx"], data["iso"])[0]
    pipe_env(monkeypatch, 0, False)
    st, msg, want = call(fn, args, data, n)
    assert st == 0 and np.isfinite(want["fr"]).all(), msg
    # i and the output in one block: 12 n bytes of input end 36 bytes into a page, where the output starts
    block = paged((2 * n, 3))
    block[:n] = data["i"][:n]
    assert (block.ctypes.data + 12 * n) % 4096 != 0
    place = {"i": (block[:n], block.ctypes.data, 3), "fr": (block[n:], block.ctypes.data + 12 * n, 3)}
    pipe_env(monkeypatch, CHUNK, True)
    st, msg, _ = call(fn, args, data, n, place=place)
    assert (st, msg) == (INVALID, "djb_error: chunked host path not taken: an input shares a host page with an output")
    pipe_env(monkeypatch, CHUNK, False)
    st, msg, got = call(fn, args, data, n, place=place)
    assert st == 0, msg
    assert np.array_equal(got["fr"].view(np.uint32), want["fr"].view(np.uint32))
    assert np.array_equal(block[:n].view(np.uint32), data["i"][:n].view(np.uint32)), "the input was written"


@pytest.mark.parametrize("padded", ["i", "fr"])
def test_a_padded_stride_is_refused(data, monkeypatch, padded):
    n = N_TAIL
    tag, fn, args = eval_calls(data, data["ggx"], data["iso"])[0]
    pipe_env(monkeypatch, 0, False)
    st, msg, want = call(fn, args, data, n)
    assert st == 0 and np.isfinite(want["fr"]).all(), msg
    rec = paged((n, 4), 7.0)                       # float4 records
    if padded == "i": rec[:, :3] = data["i"][:n]
    place = {padded: (rec, rec.ctypes.data, 4)}
    pipe_env(monkeypatch, CHUNK, True)
    st, msg, _ = call(fn, args, data, n, place=place)
    assert (st, msg) == (INVALID, "djb_error: chunked host path not taken: exotic stride (packed on the host)")
    pipe_env(monkeypatch, CHUNK, False)
    st, msg, got = call(fn, args, data, n, place=place)
    assert st == 0, msg
    assert np.array_equal(got["fr"].view(np.uint32), want["fr"].view(np.uint32))
    assert (rec[:, 3] == 7.0).all(), "the padding was written"


# ------------------------------------------------------------------ 3. null arrays on a large host batch
VIEW, INPUT, OUT_VIEW, OUT_ARR, ARG = ("djb_error: null vec3 view", "djb_error: null input array", "djb_error: null output vec3 view",
                                       "djb_error: null output array", "djb_error: null argument")
OUT_FR = "djb_error: null out_fr (the pdf alone: djb_pdf_batch)"
OUT_PDF = "djb_error: null out_pdf (evalp alone: djb_evalp_batch)"
# per body: the message for each array when that array alone is null, in the order in which the body reports them (the first entry is
# also what a call with every array null reports).  None: the array is optional, the call succeeds without it.
NULL_MESSAGES = {
    "eval": [("i", VIEW), ("o", VIEW), ("fr", OUT_VIEW)],
    "pdf": [("i", VIEW), ("o", VIEW), ("pdf", OUT_ARR)],
    "evalp+pdf": [("i", VIEW), ("o", VIEW), ("fr", OUT_VIEW), ("pdf", OUT_ARR)],
    "sample": [("u1", INPUT), ("u2", INPUT), ("o", VIEW), ("i_out", OUT_VIEW)],
    "evalp_is": [("u1", INPUT), ("u2", INPUT), ("o", VIEW), ("i_out", OUT_VIEW), ("w", OUT_VIEW), ("pdf", OUT_ARR)],
    "evalp_is_proxy": [("u1", INPUT), ("u2", INPUT), ("o", VIEW), ("i_out", OUT_VIEW), ("w", OUT_VIEW), ("pdf", OUT_ARR)],
    "evalp_pdf_proxy": [("fr", OUT_FR), ("pdf", OUT_PDF), ("i", VIEW), ("o", VIEW)],
    "eval_pp/5": [("pp", ARG), ("li", VIEW), ("lo", VIEW), ("fr", OUT_VIEW), ("pdf", OUT_ARR)],
    "eval_lean/6": [("lean", ARG), ("li", VIEW), ("lo", VIEW), ("fr", OUT_VIEW), ("pdf", OUT_ARR), ("pp_out", None)],
    "sample_pp/sample": [("lu1", ARG), ("lu2", ARG), ("pp", ARG), ("lo", VIEW), ("i_out", OUT_VIEW)],
    "sample_pp/is": [("lu1", ARG), ("lu2", ARG), ("pp", ARG), ("pdf", ARG), ("lo", VIEW), ("i_out", OUT_VIEW), ("w", None)],
    "sample_lean/is+params": [("lu1", ARG), ("lu2", ARG), ("lean", ARG), ("pdf", ARG), ("lo", VIEW), ("i_out", OUT_VIEW), ("w", None),
                              ("pp_out", None)],
}


def test_null_arrays_on_a_large_host_batch(data, monkeypatch):
    pipe_env(monkeypatch, CHUNK, False)
    d, b = data, data["beckmann"]
    bodies = eval_calls(d, d["ggx"], d["iso"]) + sample_calls(d, d["ggx"], d["ell"]) + proxy_calls(d, d["merl"], d["p_ggx"], d["iso"]) + \
        [eval_pp_call(d, b, 5), eval_lean_call(d, b, 6), sample_pp_call(d, b, False), sample_pp_call(d, b, True),
         sample_lean_call(d, b, True, True)]
    seen = set()
    for tag, fn, args in bodies:
        if tag not in NULL_MESSAGES: continue
        seen.add(tag)
        table = NULL_MESSAGES[tag]
        arrays = [a[1] for a in args if isinstance(a, tuple)]
        assert sorted(arrays) == sorted(name for name, _ in table), (tag, "the table names every array of the call")
        for name, want in table:
            st, msg, _ = call(fn, args, d, N_TAIL, null=(name,))
            assert (st, msg) == ((INVALID, want) if want else (0, "")), (tag, name, st, msg)
        st, msg, _ = call(fn, args, d, N_TAIL, null=tuple(arrays))
        assert (st, msg) == (INVALID, table[0][1]), (tag, "every array null", st, msg)
    assert seen == set(NULL_MESSAGES)
