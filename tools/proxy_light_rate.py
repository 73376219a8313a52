#!/usr/bin/env python3
"""proxy_light_rate.py -- rate of the light-sample call on one MI355X, written to profiles/proxy_light/rate.json.

    python tools/proxy_light_rate.py [--n PAIRS] [--repeats R] [--warmup W] [--out FILE]

For each of four pairs -- merl <- ggx with the parameters fitted to it (tabular(merl, 90)), abc <- tabular(abc, 90),
sgd <- tabular(sgd, 90), utia <- tabular_anisotropic(utia, 90, 90) -- it times, on n dense device-resident pairs (i and o from
gen_directions, all above the horizon):
  fused     djb_evalp_pdf_proxy_batch                                  (one kernel; 40 B per pair: i, o in; fr, pdf out)
  two_call  djb_evalp_batch on the target + djb_pdf_batch on the proxy  (36 + 28 = 64 B per pair)
  guard     the caller's guard pass behind the two calls, a torch `where` on fr and on pdf, timed on its own and reported separately
All legs run on this build in one process.

Method (the measuring guide's): everything resident in HBM; the legs alternated (fused, two_call, guard, fused, two_call, guard), W
warm-up calls and R / 2 timed calls per turn, each between two HIP events on the context's stream (djb_timer_start /
djb_timer_stop_ms): R timed calls per leg.  Median, min, max and `spread` = (max - min) / median are reported.  No speed-up is fixed
in advance: the fused leg `holds` when its median is not above the two-call median (the guard pass NOT counted) by more than the
larger of the two legs' spreads.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = ("merl_ggx_fitted", "abc_tabular", "sgd_tabular", "utia_tabular_aniso")
# guard: the mask (8 B read, 1 written) and two `where` passes (1 + 12 read, 12 written; 1 + 4 read, 4 written)
BYTES = {"fused": 40, "two_call": 64, "guard": 43}


def objects(pair, ctx):
    from dj_brdf_amd import djb, synth
    if pair == "merl_ggx_fitted":
        m = djb.merl.from_table(synth.merl_table(0.3), ctx=ctx)
        return m, djb.ggx(ctx=ctx), djb.tabular.fit_ggx_parameters(djb.tabular(m, 90, True, ctx=ctx))
    if pair == "abc_tabular":
        a = djb.abc("gold-metallic-paint", ctx=ctx)
        return a, djb.tabular(a, 90, True, ctx=ctx), None
    if pair == "sgd_tabular":
        s = djb.sgd("gold-metallic-paint", ctx=ctx)
        return s, djb.tabular(s, 90, True, ctx=ctx), None
    u = djb.utia.from_table(synth.utia_table_smooth(), ctx=ctx)
    return u, djb.tabular_anisotropic(u, 90, 90, True, ctx=ctx), None


def summarise(ms, n, leg):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4),
            "timed_calls": len(ms), "Gpairs_per_s": round(n / med / 1e6, 3), "bytes_per_pair": BYTES[leg],
            "algorithmic_GBps": round(n * BYTES[leg] / med / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=20, help="timed calls per leg, in two turns")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proxy_light", "rate.json"))
    args = ap.parse_args()
    assert args.repeats >= 20 and args.repeats % 2 == 0, "at least 20 timed calls per leg"
    import torch
    from dj_brdf_amd import _lib, djb, synth
    lib = _lib.load()
    ctx = djb.default_context(0)
    dev, n = "cuda:0", args.n
    i, o = djb.gen_directions(n, synth.SEED_I, ctx=ctx), djb.gen_directions(n, synth.SEED_O, ctx=ctx)
    i[2].abs_(); o[2].abs_()               # every pair above the horizon (the sign of a zero is cleared)
    fr = torch.empty((3, n), dtype=torch.float32, device=dev)
    pdf = torch.empty((n,), dtype=torch.float32, device=dev)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    vi, vo, vfr = djb._Vec(i), djb._Vec(o), djb._Vec(fr)
    ppdf = C.c_void_p(pdf.data_ptr())
    res = {"n": n, "timing": "HIP events around each call; legs alternated in one process, one build",
           "library": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH), "pairs": {}}
    for pair in PAIRS:
        target, proxy, params = objects(pair, ctx)
        pp = djb._params_ptr(params)

        def fused():
            _lib.check(lib.djb_evalp_pdf_proxy_batch(ctx._h, target._h, proxy._h, C.c_int64(n), C.byref(vi.view), C.byref(vo.view), None, pp,
                                                     C.byref(vfr.view), ppdf, C.c_int(0)))

        def two_call():
            _lib.check(lib.djb_evalp_batch(ctx._h, target._h, C.c_int64(n), C.byref(vi.view), C.byref(vo.view), None, C.byref(vfr.view), C.c_int(0)))
            _lib.check(lib.djb_pdf_batch(ctx._h, proxy._h, C.c_int64(n), C.byref(vi.view), C.byref(vo.view), pp, ppdf, C.c_int(0)))

        def guard():                       # the caller's pass: i.z <= 0 || o.z <= 0 -> 0 (a NaN z is not taken)
            below = (i[2] <= 0) | (o[2] <= 0)
            torch.where(below, zero, fr, out=fr)
            torch.where(below, zero, pdf, out=pdf)
        legs = {"fused": fused, "two_call": two_call, "guard": guard}
        ms = {leg: [] for leg in legs}
        for _ in range(2):                 # alternate the legs, so that drift of the machine falls on all of them
            for leg, step in legs.items():
                for _ in range(args.warmup):
                    step()
                ctx.synchronize(); torch.cuda.synchronize()
                for _ in range(args.repeats // 2):
                    ctx.timer_start(); step(); ms[leg].append(ctx.timer_stop_ms())
        s = {leg: summarise(ms[leg], n, leg) for leg in legs}
        noise = max(s["fused"]["spread"], s["two_call"]["spread"])
        entry = dict(s)
        entry["two_call_over_fused"] = round(s["two_call"]["ms_median"] / s["fused"]["ms_median"], 3)
        entry["two_call_plus_guard_over_fused"] = round((s["two_call"]["ms_median"] + s["guard"]["ms_median"]) / s["fused"]["ms_median"], 3)
        entry["larger_spread"] = noise
        entry["fused_holds"] = bool(s["fused"]["ms_median"] <= s["two_call"]["ms_median"] * (1 + noise))
        if pair == "merl_ggx_fitted":
            m = min(n, 10_000_000)
            g = djb.merl_guard_stats(i[:, :m].contiguous(), o[:, :m].contiguous(), ctx=ctx)
            entry["merl_left_tier1_share"] = (g["special"] + g["ambiguous"]) / m
            entry["ggx_fitted_params"] = [float(x) for x in params.get_ellipse()]
        res["pairs"][pair] = entry
        print(pair, json.dumps(entry), flush=True)
        del target, proxy
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    failed = [p for p, e in res["pairs"].items() if not e["fused_holds"]]
    if failed:
        sys.exit(f"proxy_light_rate: the fused call is slower than the two calls beyond the spread for {failed}")


if __name__ == "__main__":
    main()
