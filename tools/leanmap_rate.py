#!/usr/bin/env python3
"""leanmap_rate.py -- rate of the per-hit LEAN-map path on one MI355X, written to profiles/leanmap/rate.json.

    python tools/leanmap_rate.py [--n HITS] [--size TEXELS] [--repeats R] [--warmup W] [--parent-lib libdjb_hip.so] [--out FILE]

Per hit distribution -- (a) random uv in [0, 1)^2 and lod in [0, levels - 1), (b) coherent: a raster of neighbouring uv over the
map at one lod (0.5: both levels are read) -- it times, want = evalp + pdf, Beckmann with a Schlick Fresnel term, base isotropic(0.1)
(the lobe of bench.py's lean_evalp_pdf leg):
  fused     djb_eval_leanmap_batch                                      (one kernel: lookup + eval)
  two_call  djb_leanmap_lookup_batch, then djb_eval_lean_batch          (the records written to HBM and read back)
and, as the yardstick, `stream`: djb_eval_lean_batch alone on ready records -- the same arithmetic with the records streamed
instead of gathered (bench.py's lean_evalp_pdf leg, same record distribution).  With --parent-lib that leg is also timed on
another build of the library (the parent commit's), alternating with this build's in fresh processes, to show that the existing
kernels did not slow down when the per-pair kernels gained their third mode.

Method (the measuring guide's): everything resident in HBM, W warm-up calls, then R >= 10 timed calls, each between two HIP events
on the context's stream (djb_timer_start / djb_timer_stop_ms); median, min and max per leg are reported, and `spread` = (max - min)
/ median is the run-to-run noise a comparison between legs has to exceed.  Each leg's figure comes with the bytes-per-hit model
it is divided by: `streamed` bytes are the arrays every hit reads and writes once; `gathered` bytes are the 32-byte sectors of the
taps (4 per level read), which the caches may or may not absorb -- they are listed, not added to the GB/s figure.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODEL = {   # bytes per hit
    "stream":   {"streamed": 60, "gathered": 0, "what": "i 12 + o 12 + record 20 + fr 12 + pdf 4"},
    "fused":    {"streamed": 52, "gathered_per_level": 128, "what": "i 12 + o 12 + uv 8 + lod 4 + fr 12 + pdf 4; 4 taps x 32 B per level read"},
    "two_call": {"streamed": 92, "gathered_per_level": 128, "what": "lookup: uv 8 + lod 4 + record 20 written; eval: 60; 4 taps x 32 B per level read"},
}


def summarise(ms, n, leg):
    med = statistics.median(ms)
    m = dict(MODEL[leg])
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4),
            "repeats": len(ms), "Ghits_per_s": round(n / med / 1e6, 3), "streamed_GBps": round(n * m["streamed"] / med / 1e6, 1), "bytes_per_hit_model": m}


def child(args):
    import numpy as np
    import torch
    from dj_brdf_amd import _lib
    if args.child == "stream":       # may run on a build of the library that predates LEAN maps
        probe = C.CDLL(_lib.LIB_PATH)
        _lib.EXPORTS = [e for e in _lib.EXPORTS if hasattr(probe, e)]
    from dj_brdf_amd import djb, synth
    lib = _lib.load()
    ctx = djb.default_context(0)
    dev, n = "cuda:0", args.n
    b = djb.beckmann(djb.fresnel.schlick((1.0, 0.71, 0.29)), True, ctx=ctx)
    base = djb.microfacet.params.isotropic(0.1)
    i, o = djb.gen_directions(n, synth.SEED_I, ctx=ctx), djb.gen_directions(n, synth.SEED_O, ctx=ctx)
    out, pdf = torch.empty((3, n), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev)
    vi, vo, vout = djb._Vec(i), djb._Vec(o), djb._Vec(out)
    rec = torch.empty((n, 5), dtype=torch.float32, device=dev)

    def timed(step):
        for _ in range(args.warmup):
            step()
        ctx.synchronize()
        ms = []
        for _ in range(args.repeats):
            ctx.timer_start(); step(); ms.append(ctx.timer_stop_ms())
        return ms

    def eval_lean():
        _lib.check(lib.djb_eval_lean_batch(ctx._h, b._h, C.c_int64(n), C.byref(vi.view), C.byref(vo.view), C.byref(base._p), C.c_float(1.0), C.c_int(0),
                                           C.c_void_p(rec.data_ptr()), C.c_int(6), C.byref(vout.view), C.c_void_p(pdf.data_ptr()), None, C.c_int(0)))
    res = {}
    g = torch.Generator(device=dev); g.manual_seed(7)
    if args.child == "stream":       # bench.py's lean_evalp_pdf records
        rec[:, 0:2] = (torch.rand((n, 2), generator=g, device=dev) - 0.5) * 0.2
        rec[:, 2:4] = torch.rand((n, 2), generator=g, device=dev) * 0.05 + 0.01
        rec[:, 4] = (torch.rand((n,), generator=g, device=dev) - 0.5) * 0.01
        res["stream"] = summarise(timed(eval_lean), n, "stream")
        res["library"] = os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH)
        print("RESULT " + json.dumps(res))
        return
    rng = np.random.default_rng(3)
    dmap = (127 + 60 * np.sin(np.arange(args.size)[None, :] * 0.37) * np.cos(np.arange(args.size)[:, None] * 0.23)
            + rng.integers(-20, 21, (args.size, args.size))).astype(np.uint8)
    m = djb.leanmap.from_dmap(dmap, 0.05, 1e-5, ctx=ctx)
    uv, lod = torch.empty((n, 2), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev)

    def fused():
        _lib.check(lib.djb_eval_leanmap_batch(ctx._h, b._h, m._h, C.c_int64(n), C.byref(vi.view), C.byref(vo.view), C.c_void_p(uv.data_ptr()),
                                              C.c_void_p(lod.data_ptr()), C.byref(base._p), C.c_float(1.0), C.c_int(0), C.c_int(6), C.byref(vout.view),
                                              C.c_void_p(pdf.data_ptr()), None, C.c_int(0)))

    def two_call():
        _lib.check(lib.djb_leanmap_lookup_batch(ctx._h, m._h, C.c_int64(n), C.c_void_p(uv.data_ptr()), C.c_void_p(lod.data_ptr()), C.c_void_p(rec.data_ptr()), C.c_int(0)))
        eval_lean()
    side = int(round(n ** 0.5))
    for dist in ("random", "coherent"):
        if dist == "random":
            uv.copy_(torch.rand((n, 2), generator=g, device=dev)); lod.copy_(torch.rand((n,), generator=g, device=dev) * (m.levels - 1))
            levels_read = 2.0
        else:                        # pixel k of a side x side raster over the map, row by row
            k = torch.arange(n, device=dev)
            uv[:, 0] = ((k % side).float() + 0.5) / side; uv[:, 1] = ((k // side).float() + 0.5) / side
            del k
            lod.fill_(0.5)
            levels_read = 2.0
        # alternate the two legs, twice each, so that drift of the machine falls on both
        ms = {"fused": [], "two_call": []}
        for _ in range(2):
            for leg, step in (("fused", fused), ("two_call", two_call)):
                ms[leg] += timed(step)
        for leg in ms:
            r = summarise(ms[leg], n, leg)
            r["bytes_per_hit_model"]["gathered"] = int(MODEL[leg]["gathered_per_level"] * levels_read)
            res[f"{leg}_{dist}"] = r
        noise = max(res[f"fused_{dist}"]["spread"], res[f"two_call_{dist}"]["spread"])
        res[f"fused_not_slower_than_two_call_{dist}"] = bool(res[f"fused_{dist}"]["ms_median"] <= res[f"two_call_{dist}"]["ms_median"] * (1 + noise))
    res["map"] = {"size": [m.width, m.height], "levels": m.levels, "MiB": round(sum((m.width >> l or 1) * (m.height >> l or 1) for l in range(m.levels)) * 32 / 2**20, 1)}
    print("RESULT " + json.dumps(res))


def run_child(kind, args, lib_path=None):
    env = dict(os.environ)
    if lib_path:
        env["DJB_LIB_PATH"] = os.path.abspath(lib_path)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--n", str(args.n), "--size", str(args.size), "--repeats", str(args.repeats),
           "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        # whatever failed, nothing more is started on the device by this tool
        sys.exit(f"leanmap_rate: the {kind} process ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leanmap", "rate.json"))
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    assert args.repeats >= 10 or args.child, "at least 10 timed repeats"
    if args.child:
        return child(args)
    res = {"n": args.n, "want": "evalp+pdf", "lobe": "beckmann, schlick(1, 0.71, 0.29), base isotropic(0.1)", "timing": "HIP events around each call"}
    res.update(run_child("map", args))
    streams = {"this": [run_child("stream", args)]}
    if args.parent_lib:
        streams["parent"] = [run_child("stream", args, args.parent_lib)]
        streams["this"].append(run_child("stream", args))
        streams["parent"].append(run_child("stream", args, args.parent_lib))
    res["stream_this_commit"] = [s["stream"] for s in streams["this"]]
    if args.parent_lib:
        res["stream_parent_commit"] = [s["stream"] for s in streams["parent"]]
    best = min(s["ms_median"] for s in res["stream_this_commit"])
    for dist in ("random", "coherent"):
        res[f"fused_{dist}_over_stream"] = round(res[f"fused_{dist}"]["ms_median"] / best, 3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
