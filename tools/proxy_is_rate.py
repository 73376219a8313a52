#!/usr/bin/env python3
"""proxy_is_rate.py -- rate of proxy importance sampling on one MI355X, written to profiles/proxy_is/rate.json.

    python tools/proxy_is_rate.py [--n UNITS] [--repeats R] [--warmup W] [--parent-lib libdjb_hip.so] [--out FILE]

For each of three pairs -- merl <- ggx with the parameters fitted to it (tabular(merl, 90)), abc <- tabular(abc, 90),
utia <- tabular_anisotropic(utia, 90, 90) -- it times, on n dense device-resident units (o from gen_directions with o.z > 0,
uniforms from gen_uniforms):
  fused       djb_evalp_is_proxy_batch                                              (one kernel; 48 B per unit: u1, u2, o in; weight, i, pdf out)
  three_call  djb_sample_batch + djb_pdf_batch on the proxy, djb_evalp_batch on the target, one torch division pass
              (32 + 28 + 36 + 28 = 124 B per unit)
The three-call leg runs on the library given by --parent-lib (the parent commit's build), so the baseline is never the code under
test; without the option it runs on this build and the output says so.

Method (the measuring guide's): everything resident in HBM, the legs alternated in fresh processes (fused, three_call, fused,
three_call), W warm-up calls and R timed calls per process and pair, each between two HIP events on the context's stream
(djb_timer_start / djb_timer_stop_ms): 2 R timed calls per leg.  Median, min, max and `spread` = (max - min) / median are reported;
the fused leg `clears the bar` when its median is below the three-call median by more than the larger of the two spreads.
The share of the MERL pairs that leave tier 1 (djb_merl_guard_stats on the sampled pairs) is recorded with the merl pair.
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

PAIRS = ("merl_ggx_fitted", "abc_tabular", "utia_tabular_aniso")
BYTES = {"fused": 48, "three_call": 124}


def objects(pair, ctx):
    from dj_brdf_amd import djb, synth
    if pair == "merl_ggx_fitted":
        m = djb.merl.from_table(synth.merl_table(0.3), ctx=ctx)
        return m, djb.ggx(ctx=ctx), djb.tabular.fit_ggx_parameters(djb.tabular(m, 90, True, ctx=ctx))
    if pair == "abc_tabular":
        a = djb.abc("gold-metallic-paint", ctx=ctx)
        return a, djb.tabular(a, 90, True, ctx=ctx), None
    u = djb.utia.from_table(synth.utia_table_smooth(), ctx=ctx)
    return u, djb.tabular_anisotropic(u, 90, 90, True, ctx=ctx), None


def child(args):
    import torch
    from dj_brdf_amd import _lib
    probe = C.CDLL(_lib.LIB_PATH)          # the three-call leg may run on a build that predates the fused entry point
    _lib.EXPORTS = [e for e in _lib.EXPORTS if hasattr(probe, e)]
    from dj_brdf_amd import djb, synth
    lib = _lib.load()
    ctx = djb.default_context(0)
    dev, n = "cuda:0", args.n
    o = djb.gen_directions(n, synth.SEED_O, ctx=ctx)
    o[2].abs_()                            # o.z > 0 (gen_directions draws the upper hemisphere; the sign of a zero is cleared)
    u1, u2 = djb.gen_uniforms(n, synth.SEED_U1, ctx=ctx), djb.gen_uniforms(n, synth.SEED_U2, ctx=ctx)
    w, i = torch.empty((3, n), dtype=torch.float32, device=dev), torch.empty((3, n), dtype=torch.float32, device=dev)
    pdf = torch.empty((n,), dtype=torch.float32, device=dev)
    fr = torch.empty((3, n), dtype=torch.float32, device=dev) if args.child == "three_call" else None
    vo, vw, vi = djb._Vec(o), djb._Vec(w), djb._Vec(i)
    vfr = djb._Vec(fr) if fr is not None else None
    p1, p2, ppdf = C.c_void_p(u1.data_ptr()), C.c_void_p(u2.data_ptr()), C.c_void_p(pdf.data_ptr())
    res = {"library": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH)}
    for pair in PAIRS:
        target, proxy, params = objects(pair, ctx)
        pp = djb._params_ptr(params)

        def fused():
            _lib.check(lib.djb_evalp_is_proxy_batch(ctx._h, target._h, proxy._h, C.c_int64(n), p1, p2, C.byref(vo.view), None, pp,
                                                    C.byref(vw.view), C.byref(vi.view), ppdf, C.c_int(0)))

        def three_call():
            _lib.check(lib.djb_sample_batch(ctx._h, proxy._h, C.c_int64(n), p1, p2, C.byref(vo.view), pp, C.byref(vi.view), C.c_int(0)))
            _lib.check(lib.djb_pdf_batch(ctx._h, proxy._h, C.c_int64(n), C.byref(vi.view), C.byref(vo.view), pp, ppdf, C.c_int(0)))
            _lib.check(lib.djb_evalp_batch(ctx._h, target._h, C.c_int64(n), C.byref(vi.view), C.byref(vo.view), None, C.byref(vfr.view), C.c_int(0)))
            torch.div(fr, pdf, out=w)      # the caller's division pass: fr 12 + pdf 4 read, weight 12 written
        step = fused if args.child == "fused" else three_call
        for _ in range(args.warmup):
            step()
        ctx.synchronize(); torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            ctx.timer_start(); step(); ms.append(ctx.timer_stop_ms())
        res[pair] = {"ms": ms}
        if pair == "merl_ggx_fitted" and args.child == "fused":
            m = min(n, 10_000_000)         # the pairs the kernel just looked up (every 10th million suffices for a share)
            s = djb.merl_guard_stats(i[:, :m].contiguous(), o[:, :m].contiguous(), ctx=ctx)
            res[pair]["merl_left_tier1_share"] = (s["special"] + s["ambiguous"]) / m
            res[pair]["merl_guard_stats"] = {k: (list(v) if isinstance(v, tuple) else int(v)) for k, v in s.items()}
            res[pair]["ggx_fitted_params"] = [float(x) for x in params.get_ellipse()]
        del target, proxy
    print("RESULT " + json.dumps(res))


def run_child(kind, args, lib_path=None):
    env = dict(os.environ)
    if lib_path:
        env["DJB_LIB_PATH"] = os.path.abspath(lib_path)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--n", str(args.n), "--repeats", str(args.repeats), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        # whatever failed, nothing more is started on the device by this tool
        sys.exit(f"proxy_is_rate: the {kind} process ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def summarise(ms, n, leg):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4),
            "timed_calls": len(ms), "Gunits_per_s": round(n / med / 1e6, 3), "bytes_per_unit": BYTES[leg],
            "algorithmic_GBps": round(n * BYTES[leg] / med / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=10, help="timed calls per process; every leg runs in two processes")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proxy_is", "rate.json"))
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    assert args.repeats >= 10, "at least 10 timed calls per process (20 per leg)"
    runs = {"fused": [], "three_call": []}
    for _ in range(2):                     # alternate the legs, so that drift of the machine falls on both
        runs["fused"].append(run_child("fused", args))
        runs["three_call"].append(run_child("three_call", args, args.parent_lib))
    res = {"n": args.n, "timing": "HIP events around each call; legs alternated in fresh processes",
           "three_call_library": runs["three_call"][0]["library"] if args.parent_lib else "this build (no --parent-lib given)",
           "fused_library": runs["fused"][0]["library"], "pairs": {}}
    for pair in PAIRS:
        legs = {leg: summarise([m for r in runs[leg] for m in r[pair]["ms"]], args.n, leg) for leg in runs}
        noise = max(legs["fused"]["spread"], legs["three_call"]["spread"])
        ratio = legs["three_call"]["ms_median"] / legs["fused"]["ms_median"]
        entry = {"fused": legs["fused"], "three_call": legs["three_call"], "three_call_over_fused": round(ratio, 3), "larger_spread": noise,
                 "fused_clears_the_bar": bool(legs["fused"]["ms_median"] < legs["three_call"]["ms_median"] * (1 - noise))}
        for k in ("merl_left_tier1_share", "merl_guard_stats", "ggx_fitted_params"):
            if k in runs["fused"][0][pair]:
                entry[k] = runs["fused"][0][pair][k]
        res["pairs"][pair] = entry
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
