"""What the GPU tests of the per-hit families share: the arrays of one C-ABI call in a layout, with a canary unit behind every output
(Arrays), and the graph-capture protocol (graph_replay).  A family's test module writes its _call -- the entry point and its argument
order, over an Arrays -- and its cases; tests/test_hit_calls.py shows that the checks made here can fail."""
import ctypes as C

import numpy as np

from dj_brdf_amd import _lib

CANARY = np.float32(-777.25)


def dev(ctx):
    return f"cuda:{ctx.device}"


def view(ptr, n_alloc, layout):
    v = _lib.Vec3View()
    if layout == "dense":                         # [3, n_alloc]
        v.x, v.y, v.z, v.stride = ptr, ptr + 4 * n_alloc, ptr + 8 * n_alloc, 1
    else:                                         # [n_alloc, 3]
        v.x, v.y, v.z, v.stride = ptr, ptr + 4, ptr + 8, 3
    return v


class Arrays:
    """the arrays of one call in one layout ("host", "dense", "strided"): inputs as given, every output n + 1 units long with a canary in
    the last one.  vec_in / arr_in return the handle to pass (a Vec3View, for C.byref; a c_void_p), vec_out / arr_out the argument itself"""

    def __init__(self, ctx, n, layout, device=None):
        self.ctx, self.n, self.layout, self.host = ctx, n, layout, layout == "host"
        self.mem = _lib.MEM_HOST if self.host else _lib.MEM_DEVICE
        self.device = None if self.host else device or dev(ctx)
        self.ins, self.outs = [], {}              # [(handle, array)], {name: array}

    def _put(self, a):
        if self.host:
            return a, a.ctypes.data
        import torch
        t = torch.from_numpy(a).to(self.device)
        return t, t.data_ptr()

    def _shape(self, n_alloc):
        return (3, n_alloc) if self.layout == "dense" else (n_alloc, 3)

    def _full(self, shape):
        if self.host:
            a = np.full(shape, CANARY, np.float32)
            return a, a.ctypes.data
        import torch
        t = torch.full(shape, float(CANARY), dtype=torch.float32, device=self.device)
        return t, t.data_ptr()

    def vec_in(self, a):
        a = np.asarray(a)
        t, ptr = self._put(np.array(a.T if self.layout == "dense" else a, dtype=np.float32, order="C"))      # a writable copy
        self.ins.append((view(ptr, self.n, "strided" if self.host else self.layout), t))
        return self.ins[-1][0]

    def arr_in(self, a, dtype=np.float32):
        t, ptr = self._put(np.array(a, dtype))    # a writable copy: the cases' arrays are read-only
        self.ins.append((C.c_void_p(ptr), t))
        return self.ins[-1][0]

    def vec_out(self, name):
        self.outs[name], ptr = self._full(self._shape(self.n + 1))
        return C.byref(view(ptr, self.n + 1, "strided" if self.host else self.layout))

    def arr_out(self, name):
        self.outs[name], ptr = self._full((self.n + 1,))
        return C.c_void_p(ptr)

    def _back(self, t):
        h = t if self.host else t.cpu().numpy()
        return h.T if h.ndim == 2 and self.layout == "dense" else h

    def _sync(self):
        if not self.host and not str(self.device).startswith("cpu"):
            import torch
            torch.cuda.synchronize()

    def results(self, tag):
        """{output name: [n, 3] | [n]}, after the canary behind each output was checked"""
        self._sync()
        res = {}
        for name, t in self.outs.items():
            h = self._back(t)
            assert (h[self.n] == CANARY).all(), f"{tag}, {self.layout}, n = {self.n}: the unit behind output {name} was written"
            res[name] = np.ascontiguousarray(h[:self.n])
        return res

    def read(self, handle):
        """what an input's arrays hold now, [n, 3] | [n]: for a call that was given `handle` as an output too"""
        self._sync()
        return np.ascontiguousarray(self._back(next(t for h, t in self.ins if h is handle)))


def resident(ctx, a):
    """a case array as the device tensor a graph test keeps resident: [n, 3] -> [3, n], [n] as it is"""
    import torch
    return torch.from_numpy(np.array(a.T if a.ndim == 2 else a, order="C")).to(dev(ctx))


def loads(ctx, tensors, data):
    """per data set of `data`, the callable that copies its arrays into the resident `tensors`: graph_replay's loads"""
    return [lambda d=d: [t.copy_(resident(ctx, a)) for t, a in zip(tensors, d)] for d in data]


def graph_replay(ctx, launch, outs, loads):
    """The capture protocol on a side stream of ctx.device.  Per entry of `loads` (a callable that puts one data set into the resident
    inputs) a direct launch(), the first of them the warm call, and its results cloned; the outputs zeroed; launch() captured, which must
    run nothing; then per data set the outputs zeroed, the data loaded, one replay, and every tensor of `outs` held, as int32 bits,
    against its clone.  -> the clones, [data set][output]"""
    import torch
    side = torch.cuda.Stream(device=ctx.device)
    torch.cuda.synchronize()                      # the caller's tensors may have been made on another stream
    want = []
    with torch.cuda.stream(side):
        for load in loads:                        # eager: the warm call, and the results to hold the replays against
            load(); launch(); side.synchronize()
            want.append([a.clone() for a in outs])
        for a in outs:
            a.zero_()
        side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch()
    for a in outs:                                # capture executes nothing
        assert not a.any(), "a call ran during capture instead of being recorded"
    for k, load in enumerate(loads):
        with torch.cuda.stream(side):
            for a in outs:                        # a replay that runs nothing shows on a data set that is loaded twice, too
                a.zero_()
            load()
        side.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for j, (a, e) in enumerate(zip(outs, want[k])):
            assert torch.equal(a.view(torch.int32), e.view(torch.int32)), f"graph replay {k} differs from the direct call: output {j}"
    return want
