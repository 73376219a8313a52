#!/usr/bin/env python3
"""scene_proxy_rate.py -- rate of the two per-hit proxy calls of a scene on one MI355X against the route a caller has without them,
written to profiles/scene_proxy/rate.json.

    python tools/scene_proxy_rate.py [--n HITS] [--repeats R] [--warmup W] [--materials M] [--out FILE]

M = 16 materials PER KIND -- MERL and UTIA members from the synthetic tables of tools/scene_rate.py (four contents, cycled) with one ggx
parameter set per material, sgd and abc from the published rows with their fitted tabular(90, shadowing) proxies -- a scene of 4 M slots
(slot = kind * M + local) and n dense device-resident hits (i, o from gen_directions with z > 0: all above the horizon; u1, u2 from
gen_uniforms).  For each of the two calls (sample: djb_scene_evalp_is_proxy_batch, light: djb_scene_evalp_pdf_proxy_batch) and each of
two id orders (random: kinds and materials drawn per hit; sorted: kind-major) it times
  <call>_scene_<order>     the scene call
  <call>_caller_<order>    the route a caller has with the set calls alone: a torch partition by kind (stable sort of the kinds, gathers of
                           the ids and the input streams; the four sub-batch sizes read back to the host), djb_merl_set_*, for utia a
                           FURTHER partition of its segment by material (the M sizes read back) and M single-material djb_evalp_*_proxy
                           calls, the two djb_model_set_* calls, and a scatter of every output
Method (the measuring guide's): one process, everything resident in HBM, W warm-up rounds, then R rounds in which the legs run
ALTERNATELY, each leg between two HIP events on the stream the context and torch share.  Median, min, max and spread = (max - min) /
median per leg.  Bytes per hit are COUNTED from the signatures, not measured (djb_kernels_scene_proxy.hip: 68 sampling, 60 light sample).
Nothing here is a gate.  Reads and writes nothing outside the tree."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
KINDS = ("merl", "utia", "sgd", "abc")
BYTES = {"sample": 68, "light": 60}


def summarise(ms, n, nbytes=None):
    med = statistics.median(ms)
    r = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4),
         "timed_calls": len(ms), "Ghits_per_s": round(n / med / 1e6, 3)}
    if nbytes:
        r.update({"bytes_per_hit_counted": nbytes, "algorithmic_GBps": round(n * nbytes / med / 1e6, 1)})
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--materials", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_proxy", "rate.json"))
    args = ap.parse_args()
    import torch
    import scene_rate
    from dj_brdf_amd import _lib, djb, param_tables, synth
    lib = _lib.load()
    ctx = djb.default_context(0)
    dev, n, M = "cuda:0", args.n, args.materials
    i = djb.gen_directions(n, synth.SEED_I, ctx=ctx); o = djb.gen_directions(n, synth.SEED_O, ctx=ctx)
    i[2].abs_(); o[2].abs_()
    u1 = djb.gen_uniforms(n, synth.SEED_U1, ctx=ctx); u2 = djb.gen_uniforms(n, synth.SEED_U2, ctx=ctx)
    vec = lambda: torch.empty((3, n), dtype=torch.float32, device=dev)
    sca = lambda: torch.empty((n,), dtype=torch.float32, device=dev)
    out_w, out_i, out_pdf = vec(), vec(), sca()          # the light sample writes out_w (fr) and out_pdf
    mem = C.c_int(_lib.MEM_DEVICE)
    ptr = lambda t, lo=0: C.c_void_p(t.data_ptr() + 4 * lo)

    def view(t, lo=0):
        """the SoA view of a [3, n] tensor from column lo on"""
        v = _lib.Vec3View()
        base = t.data_ptr() + 4 * lo
        v.x, v.y, v.z, v.stride = base, base + 4 * t.shape[1], base + 8 * t.shape[1], 1
        return v
    P = djb.microfacet.params
    merl_src = [djb.merl.from_table(synth.merl_table(*synth.material_recipe(m)), ctx=ctx) for m in range(4)]
    utia_src = [djb.utia.from_table(t, ctx=ctx) for t in scene_rate.utia_tables(synth)]
    utia_obj = [utia_src[m % 4] for m in range(M)]
    alphas = [0.08 + 0.5 * m / max(M - 1, 1) for m in range(M)]
    params = [P.isotropic(a) for a in alphas]
    rows = {k: np.array([getattr(param_tables, k + "_params")(name) for name in synth.MERL_NAMES], np.float64)[np.arange(M) % 100] for k in ("sgd", "abc")}
    sets = {"merl": djb.merl_set([merl_src[m % 4] for m in range(M)], params, ctx=ctx), "utia": djb.utia_set(utia_obj, ctx=ctx),
            "sgd": djb.model_set.from_rows("sgd", rows["sgd"], ctx=ctx), "abc": djb.model_set.from_rows("abc", rows["abc"], ctx=ctx)}
    sets["utia"].set_proxy_params(params)
    sets["sgd"].fit_proxy(90, True); sets["abc"].fit_proxy(90, True)
    whole = djb.scene(slots=[(k, m) for k in KINDS for m in range(M)], ctx=ctx, **sets)
    lobe = djb.ggx(ctx=ctx)
    g = torch.Generator(device=dev); g.manual_seed(8765 + M)
    ids = {"random": (torch.randint(0, 4, (n,), generator=g, device=dev, dtype=torch.int32) * M
                      + torch.randint(0, M, (n,), generator=g, device=dev, dtype=torch.int32)).contiguous()}
    ids["sorted"] = torch.sort(ids["random"]).values.contiguous()

    def scene_call(call, which):
        if call == "sample":
            _lib.check(lib.djb_scene_evalp_is_proxy_batch(ctx._h, whole._h, lobe._h, C.c_int64(n), ptr(which), ptr(u1), ptr(u2), C.byref(view(o)),
                                                          C.byref(view(out_w)), C.byref(view(out_i)), ptr(out_pdf), mem))
        else:
            _lib.check(lib.djb_scene_evalp_pdf_proxy_batch(ctx._h, whole._h, lobe._h, C.c_int64(n), ptr(which), C.byref(view(i)), C.byref(view(o)),
                                                           C.byref(view(out_w)), ptr(out_pdf), mem))

    def caller(call, which):
        """what a renderer does with the set calls alone: split by kind, gather, the member calls (utia: split again, one call per
        material), scatter every output back"""
        kind = torch.div(which, M, rounding_mode="floor")
        order = torch.sort(kind, stable=True).indices
        counts = torch.bincount(kind, minlength=4).cpu().tolist()              # the host needs the sub-batch sizes
        sub_ids = (which[order] % M).to(torch.int32).contiguous()
        lo_u, n_u = counts[0], counts[1]
        # utia has no per-hit call: its segment is ordered by material as well
        order_u = torch.sort(sub_ids[lo_u:lo_u + n_u], stable=True).indices
        counts_u = torch.bincount(sub_ids[lo_u:lo_u + n_u], minlength=M).cpu().tolist()
        order = torch.cat([order[:lo_u], order[lo_u:lo_u + n_u][order_u], order[lo_u + n_u:]])
        sub_ids = (which[order] % M).to(torch.int32).contiguous()
        sub_o = o[:, order].contiguous()
        sub_w, sub_pdf = torch.empty_like(sub_o), torch.empty((n,), dtype=torch.float32, device=dev)
        if call == "sample":
            sub_u1, sub_u2, sub_i = u1[order].contiguous(), u2[order].contiguous(), torch.empty_like(sub_o)
        else:
            sub_i = i[:, order].contiguous()
        lo = 0
        for q, k in enumerate(KINDS):
            cnt = counts[q]
            pieces = [(lo + sum(counts_u[:m]), counts_u[m], m) for m in range(M)] if k == "utia" else [(lo, cnt, None)]
            for at, c, m in pieces:
                if not c:
                    continue
                a = (C.c_int64(c), ptr(sub_ids, at))
                if call == "sample":
                    tail = (ptr(sub_u1, at), ptr(sub_u2, at), C.byref(view(sub_o, at)))
                    outs = (C.byref(view(sub_w, at)), C.byref(view(sub_i, at)), ptr(sub_pdf, at), mem)
                    if k == "merl":
                        st = lib.djb_merl_set_evalp_is_proxy_batch(ctx._h, sets[k]._h, lobe._h, *a, *tail, *outs)
                    elif k == "utia":
                        st = lib.djb_evalp_is_proxy_batch(ctx._h, utia_obj[m]._h, lobe._h, a[0], *tail, None, C.byref(params[m]._p), *outs)
                    else:
                        st = lib.djb_model_set_evalp_is_proxy_batch(ctx._h, sets[k]._h, *a, *tail, *outs)
                else:
                    tail = (C.byref(view(sub_i, at)), C.byref(view(sub_o, at)))
                    outs = (C.byref(view(sub_w, at)), ptr(sub_pdf, at), mem)
                    if k == "merl":
                        st = lib.djb_merl_set_evalp_pdf_proxy_batch(ctx._h, sets[k]._h, lobe._h, *a, *tail, *outs)
                    elif k == "utia":
                        st = lib.djb_evalp_pdf_proxy_batch(ctx._h, utia_obj[m]._h, lobe._h, a[0], *tail, None, C.byref(params[m]._p), *outs)
                    else:
                        st = lib.djb_model_set_evalp_pdf_proxy_batch(ctx._h, sets[k]._h, *a, *tail, *outs)
                _lib.check(st)
            lo += cnt
        out_w[:, order] = sub_w
        out_pdf[order] = sub_pdf
        if call == "sample":
            out_i[:, order] = sub_i
    legs = {}
    for call in ("sample", "light"):
        for name, which in ids.items():
            legs[f"{call}_scene_{name}"] = (lambda call=call, which=which: scene_call(call, which))
            legs[f"{call}_caller_{name}"] = (lambda call=call, which=which: caller(call, which))
    # once, before the clock: both routes give the same bits
    for call in ("sample", "light"):
        scene_call(call, ids["random"]); a = [t.clone() for t in (out_w, out_pdf)]
        caller(call, ids["random"])
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, (out_w, out_pdf)))
        print(f"{call}: the caller's route gives the scene call's bits: {same}", flush=True)
        del a
    ms = {k: [] for k in legs}
    for r in range(args.warmup + args.repeats):
        for k, f in legs.items():                          # alternated: every round runs every leg once
            ctx.timer_start(); f(); t = ctx.timer_stop_ms()
            if r >= args.warmup:
                ms[k].append(t)
    res = {"n": n, "materials_per_kind": M, "proxy": "ggx, one isotropic parameter set per merl / utia material; tabular(90, shadowing) per sgd / abc row",
           "timing": "HIP events around each leg; legs alternated inside every round", "warmup_rounds": args.warmup,
           "bytes_per_hit": "counted from the signatures, not measured",
           "legs": {k: summarise(v, n, BYTES[k.split("_")[0]] if "_scene_" in k else None) for k, v in ms.items()}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
