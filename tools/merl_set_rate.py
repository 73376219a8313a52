#!/usr/bin/env python3
"""merl_set_rate.py -- rate of the MERL material-set calls on one MI355X, written to profiles/merl_set/rate.json.

    python tools/merl_set_rate.py [--n HITS] [--repeats R] [--warmup W] [--materials 1,16,128] [--out FILE]

For M in {1, 16, 128} resident synthetic MERL tables and n dense device-resident hits (i, o from gen_directions with z > 0, uniforms
from gen_uniforms, ids uniform over [0, M)) it times, for eval (evalp), for sampling and for the light sample (a GGX proxy, isotropic parameters per material):
  set_random    the set call, ids as drawn                      (40 B per hit for eval, 52 B for sampling, 44 B for the light sample)
  set_sorted    the set call, ids sorted (hits of a material are contiguous)
  partitioned   M calls of the single-material operator (djb_evalp_batch / djb_evalp_is_proxy_batch; light: djb_evalp_batch and
                djb_pdf_batch) on the slices of the sorted batch: the floor a caller-side partition could reach; the partition itself
                is not timed
  single        M = 1 only: the plain single-material call(s) on the whole batch (36 B / 48 B / 36 + 28 B per hit)
and for the light sample also the cheapest route the ABI offers without the fused call, on the ids as drawn:
  composed      djb_merl_set_eval_batch(want_cos = 1) + djb_eval_pp_batch(want = pdf) on per-hit records (40 + 48 B per hit), the
                records already expanded
  expansion     the caller's side of `composed`, timed on its own: records[k] = table[ids[k]] (5 floats per hit, a torch gather);
                composed_with_expansion is the sum of the two medians
Method (the measuring guide's): everything resident in HBM, W warm-up rounds, then R rounds in which the legs run ALTERNATELY, each leg
between two HIP events on the context's stream (djb_timer_start / djb_timer_stop_ms).  Median, min, max and spread = (max - min) / median
per leg.  Nothing here is a gate."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BYTES = {"eval": {"set": 40, "single": 36}, "sample": {"set": 52, "single": 48}, "light": {"set": 44, "single": 64, "composed": 88, "expansion": 24}}
COMPOSED = "djb_merl_set_eval_batch(want_cos=1) + djb_eval_pp_batch(want=4) on expanded per-hit pdfparams records"


def summarise(ms, n, nbytes):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4),
            "timed_calls": len(ms), "Ghits_per_s": round(n / med / 1e6, 3), "bytes_per_hit": nbytes, "algorithmic_GBps": round(n * nbytes / med / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--materials", default="1,16,128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merl_set", "rate.json"))
    args = ap.parse_args()
    import torch
    from dj_brdf_amd import _lib, djb, synth
    lib = _lib.load()
    ctx = djb.default_context(0)
    dev, n = "cuda:0", args.n
    i = djb.gen_directions(n, synth.SEED_I, ctx=ctx); o = djb.gen_directions(n, synth.SEED_O, ctx=ctx)
    i[2].abs_(); o[2].abs_()
    u1, u2 = djb.gen_uniforms(n, synth.SEED_U1, ctx=ctx), djb.gen_uniforms(n, synth.SEED_U2, ctx=ctx)
    out, wi = torch.empty((3, n), dtype=torch.float32, device=dev), torch.empty((3, n), dtype=torch.float32, device=dev)
    pdf = torch.empty((n,), dtype=torch.float32, device=dev)
    ggx = djb.ggx(ctx=ctx)
    mem = C.c_int(_lib.MEM_DEVICE)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def view(t, lo=0, m=None):
        """the SoA view of units [lo, lo + m) of a [3, n] tensor"""
        v = _lib.Vec3View()
        base = t.data_ptr() + 4 * lo
        v.x, v.y, v.z, v.stride = base, base + 4 * n, base + 8 * n, 1
        return v
    res = {"n": n, "timing": "HIP events around each leg; legs alternated inside every round", "warmup_rounds": args.warmup, "materials": {}}
    for M in [int(x) for x in args.materials.split(",")]:
        tables = [synth.merl_table(*synth.material_recipe(m)) for m in range(min(M, 4))]          # four distinct contents, cycled
        members = [djb.merl.from_table(t, ctx=ctx) for t in tables]
        alphas = [0.05 + 0.4 * ((7 * m) % 16) / 16.0 for m in range(M)]
        params = [djb.microfacet.params.isotropic(a) for a in alphas]
        mset = djb.merl_set([members[m % len(members)] for m in range(M)], params, ctx=ctx)
        g = torch.Generator(device=dev); g.manual_seed(1234 + M)
        ids = torch.randint(0, M, (n,), generator=g, device=dev, dtype=torch.int32)
        ids_sorted = torch.sort(ids).values.contiguous()
        bounds = torch.searchsorted(ids_sorted, torch.arange(M + 1, device=dev, dtype=torch.int32)).cpu().tolist()
        vi, vo, vout, vwi = view(i), view(o), view(out), view(wi)

        def set_eval(which):
            _lib.check(lib.djb_merl_set_eval_batch(ctx._h, mset._h, C.c_int64(n), ptr(which), C.byref(vi), C.byref(vo), C.c_int(1), C.byref(vout), mem))

        def set_sample(which):
            _lib.check(lib.djb_merl_set_evalp_is_proxy_batch(ctx._h, mset._h, ggx._h, C.c_int64(n), ptr(which), ptr(u1), ptr(u2), C.byref(vo), C.byref(vout),
                                                             C.byref(vwi), ptr(pdf), mem))

        def set_light(which):
            _lib.check(lib.djb_merl_set_evalp_pdf_proxy_batch(ctx._h, mset._h, ggx._h, C.c_int64(n), ptr(which), C.byref(vi), C.byref(vo), C.byref(vout),
                                                              ptr(pdf), mem))
        rec_table = torch.tensor([[a, a, 0.0, 0.0, 0.0] for a in alphas], dtype=torch.float32, device=dev)      # pdfparams of isotropic(alpha)
        ids64 = ids.long()
        rec = torch.empty((n, 5), dtype=torch.float32, device=dev)

        def expansion():
            torch.index_select(rec_table, 0, ids64, out=rec)

        def composed():
            set_eval(ids)
            _lib.check(lib.djb_eval_pp_batch(ctx._h, ggx._h, C.c_int64(n), C.byref(vi), C.byref(vo), ptr(rec), C.c_int(4), C.byref(vwi), ptr(pdf), mem))

        def part_light():
            for m in range(M):
                lo, cnt = bounds[m], bounds[m + 1] - bounds[m]
                if cnt:
                    a, b, c = view(i, lo), view(o, lo), view(out, lo)
                    _lib.check(lib.djb_evalp_batch(ctx._h, members[m % len(members)]._h, C.c_int64(cnt), C.byref(a), C.byref(b), None, C.byref(c), mem))
                    _lib.check(lib.djb_pdf_batch(ctx._h, ggx._h, C.c_int64(cnt), C.byref(a), C.byref(b), C.byref(params[m]._p),
                                                 C.c_void_p(pdf.data_ptr() + 4 * lo), mem))
        expansion()

        def part_eval():
            for m in range(M):
                lo, cnt = bounds[m], bounds[m + 1] - bounds[m]
                if cnt:
                    a, b, c = view(i, lo), view(o, lo), view(out, lo)
                    _lib.check(lib.djb_evalp_batch(ctx._h, members[m % len(members)]._h, C.c_int64(cnt), C.byref(a), C.byref(b), None, C.byref(c), mem))

        def part_sample():
            for m in range(M):
                lo, cnt = bounds[m], bounds[m + 1] - bounds[m]
                if cnt:
                    b, c, d = view(o, lo), view(out, lo), view(wi, lo)
                    _lib.check(lib.djb_evalp_is_proxy_batch(ctx._h, members[m % len(members)]._h, ggx._h, C.c_int64(cnt), C.c_void_p(u1.data_ptr() + 4 * lo),
                                                            C.c_void_p(u2.data_ptr() + 4 * lo), C.byref(b), None, C.byref(params[m]._p), C.byref(c), C.byref(d),
                                                            C.c_void_p(pdf.data_ptr() + 4 * lo), mem))
        legs = {"eval": {"set_random": lambda: set_eval(ids), "set_sorted": lambda: set_eval(ids_sorted), "partitioned": part_eval},
                "sample": {"set_random": lambda: set_sample(ids), "set_sorted": lambda: set_sample(ids_sorted), "partitioned": part_sample},
                "light": {"set_random": lambda: set_light(ids), "set_sorted": lambda: set_light(ids_sorted), "partitioned": part_light,
                          "composed": composed, "expansion": expansion}}
        if M == 1:
            for call, single in (("eval", part_eval), ("sample", part_sample), ("light", part_light)):
                legs[call]["single"] = single           # one slice: the whole batch
                del legs[call]["partitioned"]
        entry = {}
        for call, group in legs.items():
            ms = {k: [] for k in group}
            for r in range(args.warmup + args.repeats):
                for k, f in group.items():             # alternated: every round runs every leg once
                    ctx.timer_start(); f(); t = ctx.timer_stop_ms()
                    if r >= args.warmup:
                        ms[k].append(t)
            entry[call] = {k: summarise(v, n, BYTES[call].get(k, BYTES[call]["set" if k.startswith("set") else "single"])) for k, v in ms.items()}
        entry["light"]["composed"]["route"] = COMPOSED
        entry["light"]["composed_with_expansion_ms_median"] = round(entry["light"]["composed"]["ms_median"] + entry["light"]["expansion"]["ms_median"], 4)
        res["materials"][str(M)] = entry
        print(M, json.dumps(entry), flush=True)
        mset.close()
        for b in members:
            b.close()
        del ids, ids_sorted, ids64, rec
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
