#!/usr/bin/env python3
"""model_set_proxy_rate.py -- rate of the two per-hit proxy calls of an SGD / ABC model set on one MI355X, written to
profiles/model_set_proxy/rate.json.

    python tools/model_set_proxy_rate.py [--n HITS] [--repeats R] [--warmup W] [--materials 1,16,100] [--kinds sgd,abc] [--out FILE]

For each kind and M in {1, 16, 100} resident rows (the 100 published rows, cycled over the set), fitted at res 90 with shadowing, and n dense
device-resident hits (o and i from gen_directions with z > 0: all above the horizon; u1, u2 from gen_uniforms; ids uniform over [0, M)) it
times both calls -- `sample` = djb_model_set_evalp_is_proxy_batch (52 B per hit, counted from the signature), `light` =
djb_model_set_evalp_pdf_proxy_batch (44 B per hit):
  set_random    the set call, ids as drawn
  set_sorted    the set call, ids sorted (hits of a material are contiguous)
  partitioned   the route a caller has without the set: M calls of djb_evalp_is_proxy_batch / djb_evalp_pdf_proxy_batch with per-material
                tabular objects on the slices of the sorted batch; the partition itself is not timed
  single        M = 1 only, instead of `partitioned`: the plain call on the whole batch (48 / 40 B per hit)
Method (the measuring guide's): everything resident in HBM, W warm-up rounds, then R rounds in which the legs run ALTERNATELY, each leg
between two HIP events on the context's stream (djb_timer_start / djb_timer_stop_ms).  Median, min, max and spread = (max - min) / median
per leg.  Nothing here is a gate.  Reads and writes nothing outside the tree."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BYTES = {"sample": {"set": 52, "single": 48}, "light": {"set": 44, "single": 40}}
RES, SHADOW = 90, True


def summarise(ms, n, nbytes):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4),
            "timed_calls": len(ms), "Ghits_per_s": round(n / med / 1e6, 3), "bytes_per_hit": nbytes, "algorithmic_GBps": round(n * nbytes / med / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--materials", default="1,16,100")
    ap.add_argument("--kinds", default="sgd,abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_set_proxy", "rate.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from dj_brdf_amd import _lib, djb, param_tables, synth
    lib = _lib.load()
    ctx = djb.default_context(0)
    dev, n = "cuda:0", args.n
    i = djb.gen_directions(n, synth.SEED_I, ctx=ctx); o = djb.gen_directions(n, synth.SEED_O, ctx=ctx)
    i[2].abs_(); o[2].abs_()
    u1 = djb.gen_uniforms(n, synth.SEED_U1, ctx=ctx); u2 = djb.gen_uniforms(n, synth.SEED_U2, ctx=ctx)
    out_a = torch.empty((3, n), dtype=torch.float32, device=dev); out_b = torch.empty((3, n), dtype=torch.float32, device=dev)
    out_pdf = torch.empty(n, dtype=torch.float32, device=dev)
    mem = C.c_int(_lib.MEM_DEVICE)

    def view(t, lo=0):
        """the SoA view of the units from lo on of a [3, n] tensor"""
        v = _lib.Vec3View()
        base = t.data_ptr() + 4 * lo
        v.x, v.y, v.z, v.stride = base, base + 4 * n, base + 8 * n, 1
        return v

    def at(t, lo=0):
        return C.c_void_p(t.data_ptr() + 4 * lo)
    res = {"n": n, "proxy": {"res": RES, "shadow": SHADOW}, "timing": "HIP events around each leg; legs alternated inside every round",
           "warmup_rounds": args.warmup, "kinds": {}}
    for kind in args.kinds.split(","):
        look = param_tables.sgd_params if kind == "sgd" else param_tables.abc_params
        rows = np.array([look(name) for name in synth.MERL_NAMES], np.float64)
        cls = djb.sgd if kind == "sgd" else djb.abc
        n_members = min(max(int(x) for x in args.materials.split(",")), len(rows))
        members = [cls.from_params(r, ctx=ctx) for r in rows[:n_members]]
        proxies = [djb.tabular(b, RES, SHADOW, ctx=ctx) for b in members]
        res["kinds"][kind] = {}
        for M in [int(x) for x in args.materials.split(",")]:
            mset = djb.model_set.from_rows(kind, rows[np.arange(M) % len(rows)], ctx=ctx)
            mset.fit_proxy(RES, SHADOW)
            g = torch.Generator(device=dev); g.manual_seed(1234 + M)
            ids = torch.randint(0, M, (n,), generator=g, device=dev, dtype=torch.int32)
            ids_sorted = torch.sort(ids).values.contiguous()
            bounds = torch.searchsorted(ids_sorted, torch.arange(M + 1, device=dev, dtype=torch.int32)).cpu().tolist()

            def set_sample(which):
                vo, vw, vi = view(o), view(out_a), view(out_b)
                _lib.check(lib.djb_model_set_evalp_is_proxy_batch(ctx._h, mset._h, C.c_int64(n), at(which), at(u1), at(u2), C.byref(vo), C.byref(vw), C.byref(vi),
                                                                  at(out_pdf), mem))

            def set_light(which):
                vi, vo, vf = view(i), view(o), view(out_a)
                _lib.check(lib.djb_model_set_evalp_pdf_proxy_batch(ctx._h, mset._h, C.c_int64(n), at(which), C.byref(vi), C.byref(vo), C.byref(vf), at(out_pdf), mem))

            def part_sample():
                for m in range(M):
                    lo, cnt = bounds[m], bounds[m + 1] - bounds[m]
                    if cnt:
                        vo, vw, vi = view(o, lo), view(out_a, lo), view(out_b, lo)
                        _lib.check(lib.djb_evalp_is_proxy_batch(ctx._h, members[m % n_members]._h, proxies[m % n_members]._h, C.c_int64(cnt), at(u1, lo), at(u2, lo),
                                                                C.byref(vo), None, None, C.byref(vw), C.byref(vi), at(out_pdf, lo), mem))

            def part_light():
                for m in range(M):
                    lo, cnt = bounds[m], bounds[m + 1] - bounds[m]
                    if cnt:
                        vi, vo, vf = view(i, lo), view(o, lo), view(out_a, lo)
                        _lib.check(lib.djb_evalp_pdf_proxy_batch(ctx._h, members[m % n_members]._h, proxies[m % n_members]._h, C.c_int64(cnt), C.byref(vi), C.byref(vo),
                                                                 None, None, C.byref(vf), at(out_pdf, lo), mem))
            entry = {}
            for call, set_call, part_call in (("sample", set_sample, part_sample), ("light", set_light, part_light)):
                legs = {"set_random": lambda f=set_call: f(ids), "set_sorted": lambda f=set_call: f(ids_sorted), "single" if M == 1 else "partitioned": part_call}
                ms = {k: [] for k in legs}
                for r in range(args.warmup + args.repeats):
                    for k, f in legs.items():                  # alternated: every round runs every leg once
                        ctx.timer_start(); f(); t = ctx.timer_stop_ms()
                        if r >= args.warmup:
                            ms[k].append(t)
                entry[call] = {k: summarise(v, n, BYTES[call]["set" if k.startswith("set") else "single"]) for k, v in ms.items()}
            res["kinds"][kind][str(M)] = entry
            print(kind, M, json.dumps(entry), flush=True)
            mset.close()
            del ids, ids_sorted
            torch.cuda.empty_cache()
        for b in proxies + members:
            b.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
