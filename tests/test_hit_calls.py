"""tests/hit_calls.py under test: the checks the per-hit GPU modules rely on are shown to be able to fail.

On the CPU: view's pointer arithmetic; Arrays in its three layouts (dense and strided on device="cpu" tensors) against a fake call written
in Python, which reads the inputs and writes a known function of them through the views it is handed, over the addresses alone -- the
orientation of what results / read return, the canary check tripping on a vector and on a scalar output, an in-place output --; one real
call on a CPU context against the Python API.  On the GPU, with torch alone: graph_replay on a launch that replays faithfully, and on one
whose captured form differs from its direct calls."""
import ctypes as C

import numpy as np
import pytest

import model_set_cases
from dj_brdf_amd import _lib, djb
from hit_calls import CANARY, Arrays, dev, graph_replay, view

LAYOUTS = ("host", "dense", "strided")
SIZES = (1, 5, 64)


def _mem(ptr, count, ctype=C.c_float):
    """`count` elements at address `ptr`, as a numpy array over that memory"""
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (count,))


def _plane(v, k, count):
    """component k of the first `count` units that the Vec3View v names"""
    return _mem((v.x, v.y, v.z)[k], (count - 1) * v.stride + 1)[::v.stride]


def _inputs(n):
    rng = np.random.default_rng(n)
    ids = rng.integers(-1, 7, n).astype(np.int32)
    vec, sca = rng.random((n, 3), dtype=np.float32), rng.random(n, dtype=np.float32)
    for a in (ids, vec, sca):
        a.setflags(write=False)                   # as the cases' arrays are
    return ids, vec, sca


def _expected(ids, vec, sca):
    """what _fake_call writes: [n, 3] and [n]"""
    return vec * np.float32(2) + ids[:, None].astype(np.float32) + np.arange(3, dtype=np.float32), sca * np.float32(3) - ids.astype(np.float32)


def _fake_call(n, pid, vin, psca, out_vec, out_sca, spill=()):
    """a call of the C ABI's shape: ids, a vector and a scalar input; a vector and a scalar output.  spill names the outputs ("vec",
    "sca") whose unit n it writes, too"""
    ids = _mem(pid.value, n, C.c_int32)
    want_vec, want_sca = _expected(ids, np.stack([_plane(vin, k, n) for k in range(3)], 1), _mem(psca.value, n))
    for k in range(3):
        _plane(out_vec, k, n)[:] = want_vec[:, k]
        if "vec" in spill:
            _plane(out_vec, k, n + 1)[n] = k
    _mem(out_sca.value, n)[:] = want_sca
    if "sca" in spill:
        _mem(out_sca.value, n + 1)[n] = 0


def _arrays(n, layout):
    return Arrays(None, n, layout, device="cpu")


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ view
def test_view_names_planes_or_records():
    v = view(4096, 7, "dense")
    assert (v.x, v.y, v.z, v.stride) == (4096, 4096 + 4 * 7, 4096 + 8 * 7, 1)
    for layout in ("strided", "host"):
        v = view(4096, 7, layout)
        assert (v.x, v.y, v.z, v.stride) == (4096, 4100, 4104, 3)
    planes, records = np.arange(21, dtype=np.float32).reshape(3, 7), np.arange(21, dtype=np.float32).reshape(7, 3)
    for k in range(3):
        assert np.array_equal(_plane(view(planes.ctypes.data, 7, "dense"), k, 7), planes[k])
        assert np.array_equal(_plane(view(records.ctypes.data, 7, "strided"), k, 7), records[:, k])


# ------------------------------------------------------------------ Arrays against the fake call
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_results_come_back_in_the_cases_orientation(layout, n):
    ids, vec, sca = _inputs(n)
    A = _arrays(n, layout)
    assert A.mem == (_lib.MEM_HOST if layout == "host" else _lib.MEM_DEVICE)
    pid, vin, psca = A.arr_in(ids, np.int32), A.vec_in(vec), A.arr_in(sca)
    assert vin.stride == (1 if layout == "dense" else 3)
    out_vec, out_sca = A.vec_out("vec"), A.arr_out("sca")
    before = {name: np.array(A._back(t)) for name, t in A.outs.items()}
    assert before["vec"].shape == (n + 1, 3) and before["sca"].shape == (n + 1,) and all((a == CANARY).all() for a in before.values())
    _fake_call(n, pid, vin, psca, out_vec._obj, out_sca)
    got = A.results("fake")
    want_vec, want_sca = _expected(ids, vec, sca)
    assert list(got) == ["vec", "sca"] and _same_bits(got["vec"], want_vec) and _same_bits(got["sca"], want_sca)
    assert _same_bits(A.read(vin), vec) and np.array_equal(A.read(pid), ids) and A.read(pid).dtype == np.int32       # the inputs, as given


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("spilt", ["vec", "sca"])
def test_a_write_behind_an_output_fails_the_canary_check(spilt, layout, n):
    ids, vec, sca = _inputs(n)
    A = _arrays(n, layout)
    pid, vin, psca = A.arr_in(ids, np.int32), A.vec_in(vec), A.arr_in(sca)
    _fake_call(n, pid, vin, psca, A.vec_out("vec")._obj, A.arr_out("sca"), spill=(spilt,))
    with pytest.raises(AssertionError) as e:
        A.results("fake")
    msg = str(e.value)
    assert f"fake, {layout}, n = {n}: the unit behind output {spilt} was written" in msg, msg


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_an_output_over_an_input_is_read_back(layout, n):
    ids, vec, sca = _inputs(n)
    A = _arrays(n, layout)
    pid, vin, psca = A.arr_in(ids, np.int32), A.vec_in(vec), A.arr_in(sca)
    _fake_call(n, pid, vin, psca, vin, psca)          # both outputs over the inputs' arrays: no canary unit behind them
    want_vec, want_sca = _expected(ids, vec, sca)
    assert _same_bits(A.read(vin), want_vec) and _same_bits(A.read(psca), want_sca)
    assert A.results("fake") == {}


# ------------------------------------------------------------------ one real call
def test_a_real_call_on_a_cpu_context_equals_the_python_api():
    cpu = djb.cpu_context()
    s = djb.model_set.from_rows("sgd", model_set_cases.rows("sgd"), ctx=cpu)
    try:
        n = 5
        ids = np.int32([0, 1, 2, 3, -1])
        i, o = (a[:n] for a in model_set_cases.eval_inputs())
        A = Arrays(cpu, n, "host")
        pid, vi, vo = A.arr_in(ids, np.int32), A.vec_in(i), A.vec_in(o)
        _lib.check(_lib.load().djb_model_set_eval_batch(cpu._h, s._h, C.c_int64(n), pid, C.byref(vi), C.byref(vo), C.c_int(1), A.vec_out("fr"), C.c_int(A.mem)))
        got = A.results("model set on the cpu")["fr"]
        want = np.asarray(s.evalp(ids, i, o))
        assert _same_bits(got, want) and np.nansum(np.abs(want)) > 0 and not want[4].view(np.uint32).any()
    finally:
        s.close()


# ------------------------------------------------------------------ graph_replay
@pytest.mark.gpu
def test_graph_replay_passes_a_launch_that_replays_what_it_ran(gpu_ctx):
    import torch
    data = [torch.arange(64, dtype=torch.float32) + 1, -torch.arange(64, dtype=torch.float32) - 0.5]
    inp, out = (torch.zeros(64, dtype=torch.float32, device=dev(gpu_ctx)) for _ in range(2))
    want = graph_replay(gpu_ctx, lambda: out.copy_(inp * 2), [out], [lambda d=d: inp.copy_(d) for d in data])
    assert len(want) == 2 and all(len(w) == 1 and torch.equal(w[0].cpu(), d * 2) for w, d in zip(want, data))
    assert torch.equal(out.cpu(), data[1] * 2)


@pytest.mark.gpu
def test_graph_replay_fails_a_replay_that_differs_from_the_direct_call(gpu_ctx):
    """the launch fills with a Python counter: the direct calls see 1 and 2, the capture bakes in 3"""
    import torch
    out = torch.zeros(64, dtype=torch.float32, device=dev(gpu_ctx))
    calls = [0]

    def launch():
        calls[0] += 1
        out.fill_(float(calls[0]))
    with pytest.raises(AssertionError, match="graph replay 0 differs from the direct call"):
        graph_replay(gpu_ctx, launch, [out], [lambda: None] * 2)
    assert calls[0] == 3 and (out.cpu() == 3).all()
