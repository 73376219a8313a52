#!/usr/bin/env python3
"""microfacet_set_rate.py -- rate of the microfacet-set calls on one MI355X, written to profiles/microfacet_set/rate.json.

    python tools/microfacet_set_rate.py [--n HITS] [--repeats R] [--warmup W] [--materials 16,4096] [--out FILE]

For ggx eval + pdf, ggx evalp_is and beckmann evalp_is, M in {16, 4096} resident materials and n dense device-resident hits (i, o from
gen_directions with z > 0: all above the horizon; uniforms from gen_uniforms; ids uniform over [0, M), as drawn: unsorted) it times
  set_uniform   the set call on a set whose materials all carry a schlick term (the compile-time Fresnel route)
  set_mixed     the set call on the same parameter sets with the four Fresnel kinds and both shadowing flags cycled (the per-row switch)
  set_global    set_uniform under DJB_OPT_MICROFACET_SET_ROWS_GLOBAL -- only where M fits the LDS budget (ROWS_LDS)
  single        the single-material call on the same pairs with material 0: set_uniform - single is the cost of per-lane rows
  gather_pp     what a caller has without the set for a uniform-Fresnel set: records[ids] gathered with torch (n x 5 floats written, then
                read by the kernel) + djb_eval_pp_batch / djb_sample_pp_batch on one schlick object; its parts are timed too (gather,
                pp on gathered records)
  partition     M = 16 only, what a caller has for a mixed-Fresnel set: a torch partition by material (sort of the ids, gathers of the
                inputs, a read-back of the sub-batch sizes), M single-material calls on the slices, a scatter of the outputs; its parts
                are timed too (partition, calls, scatter)
Bytes per hit are counted from the signatures: set eval + pdf 4 + 24 + 16 = 44, set evalp_is 4 + 8 + 12 + 28 = 52; single 40 / 48;
gather_pp adds 4 (ids) + 20 written + 20 read to the single call's.
Method (the measuring guide's): everything resident in HBM, W warm-up rounds, then R rounds in which the legs run ALTERNATELY, each leg
between two HIP events on the context's stream (djb_timer_start / djb_timer_stop_ms; the context follows torch's current stream, so the torch work of a leg is in the same queue).
Median, min, max and spread = (max - min) / median per leg, and for each comparison the ratio of medians next to the larger spread of
the pair.  Nothing here is a gate.  Reads and writes nothing outside the tree."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS_LDS = 200
BYTES = {"eval_pdf": {"set": 44, "single": 40, "gather_pp": 84}, "evalp_is": {"set": 52, "single": 48, "gather_pp": 92}}
CONFIGS = (("ggx", "eval_pdf"), ("ggx", "evalp_is"), ("beckmann", "evalp_is"))


def summarise(ms, n, nbytes=None):
    med = statistics.median(ms)
    d = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4),
         "timed_calls": len(ms), "Ghits_per_s": round(n / med / 1e6, 3)}
    if nbytes:
        d.update(bytes_per_hit=nbytes, algorithmic_GBps=round(n * nbytes / med / 1e6, 1))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--materials", default="16,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microfacet_set", "rate.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from dj_brdf_amd import _lib, djb, synth
    lib = _lib.load()
    ctx = djb.default_context(0)
    dev, n = "cuda:0", args.n
    stream = torch.cuda.current_stream(0)                            # the context follows torch's current stream: one queue for both
    P = djb.microfacet.params
    mem = C.c_int(_lib.MEM_DEVICE)
    i = djb.gen_directions(n, synth.SEED_I, ctx=ctx); o = djb.gen_directions(n, synth.SEED_O, ctx=ctx)
    i[2].abs_(); o[2].abs_()
    u1 = djb.gen_uniforms(n, synth.SEED_U1, ctx=ctx); u2 = djb.gen_uniforms(n, synth.SEED_U2, ctx=ctx)
    vec = lambda: torch.empty((3, n), dtype=torch.float32, device=dev)
    arr = lambda: torch.empty((n,), dtype=torch.float32, device=dev)
    out_a, out_b, out_pdf = vec(), vec(), arr()                      # fr or weight, i, pdf
    si, so, s1, s2, sa, sb, spdf = vec(), vec(), arr(), arr(), vec(), vec(), arr()       # the partition's sorted copies
    torch.cuda.synchronize()

    def view(t, lo=0):
        v = _lib.Vec3View()
        base = t.data_ptr() + 4 * lo
        v.x, v.y, v.z, v.stride = base, base + 4 * n, base + 8 * n, 1
        return v

    def at(t, lo=0):
        return C.c_void_p(t.data_ptr() + 4 * lo)
    f0 = (1.0, 0.71, 0.29)
    fresnels = [djb.fresnel.schlick(f0), djb.fresnel.ideal(), djb.fresnel.unpolarized((1.5, 1.8, 2.4)), djb.fresnel.sgd((0.8, 0.5, 0.3), (0.1, 0.05, 0.02))]
    res = {"n": n, "timing": "HIP events around each leg; legs alternated inside every round", "warmup_rounds": args.warmup, "rows_lds": ROWS_LDS,
           "ids": "uniform over [0, M), unsorted", "configs": {}}
    for kind, op in CONFIGS:
        cls = djb.ggx if kind == "ggx" else djb.beckmann
        res["configs"][f"{kind} {op}"] = {}
        for M in [int(x) for x in args.materials.split(",")]:
            rng = np.random.default_rng(7 + M)
            rec = np.stack([rng.uniform(0.05, 0.6, M), rng.uniform(0.05, 0.6, M), rng.uniform(-0.5, 0.5, M), rng.uniform(-0.2, 0.2, M),
                            rng.uniform(-0.2, 0.2, M)], 1).astype(np.float32)
            params = [P.pdfparams(*[float(x) for x in r]) for r in rec]
            uniform = djb.microfacet_set.from_materials(kind, [(fresnels[0], True, p) for p in params], ctx=ctx)
            mixed = djb.microfacet_set.from_materials(kind, [(fresnels[m % 4], (m // 4) % 2 == 0, p) for m, p in enumerate(params)], ctx=ctx)
            single = cls(fresnels[0], True, ctx=ctx)
            members = [cls(fresnels[m % 4], (m // 4) % 2 == 0, ctx=ctx) for m in range(M)] if M <= 16 else []
            g = torch.Generator(device=dev); g.manual_seed(1234 + M)
            ids = torch.randint(0, M, (n,), generator=g, device=dev, dtype=torch.int32)
            ids64 = ids.long()
            records = torch.from_numpy(rec).to(dev)
            gathered = torch.empty((n, 5), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            vi, vo, va, vb = view(i), view(o), view(out_a), view(out_b)

            def set_call(s, rows_global=False):
                if rows_global:
                    djb.set_microfacet_set_rows_global(ctx, True)
                if op == "eval_pdf":
                    _lib.check(lib.djb_microfacet_set_eval_batch(ctx._h, s._h, C.c_int64(n), at(ids), C.byref(vi), C.byref(vo), C.c_int(5), C.byref(va), at(out_pdf), mem))
                else:
                    _lib.check(lib.djb_microfacet_set_sample_batch(ctx._h, s._h, C.c_int64(n), at(ids), at(u1), at(u2), C.byref(vo), C.byref(va), C.byref(vb),
                                                                   at(out_pdf), mem))
                if rows_global:
                    djb.set_microfacet_set_rows_global(ctx, False)

            def one_call(b, p, cnt, lo, src):
                """the single-material call on cnt units from lo on of the arrays src = (i, o, u1, u2, a, b, pdf)"""
                ti, to, t1, t2, ta, tb, tp = src
                a_, b_ = view(ta, lo), view(tb, lo)
                if op == "eval_pdf":
                    x, y = view(ti, lo), view(to, lo)
                    _lib.check(lib.djb_eval_pdf_batch(ctx._h, b._h, C.c_int64(cnt), C.byref(x), C.byref(y), C.byref(p._p), C.c_int(0), C.byref(a_), at(tp, lo), mem))
                else:
                    y = view(to, lo)
                    _lib.check(lib.djb_evalp_is_batch(ctx._h, b._h, C.c_int64(cnt), at(t1, lo), at(t2, lo), C.byref(y), C.byref(p._p), C.byref(a_), C.byref(b_),
                                                      at(tp, lo), mem))
            plain = (i, o, u1, u2, out_a, out_b, out_pdf)

            def gather():
                with torch.cuda.stream(stream):
                    torch.index_select(records, 0, ids64, out=gathered)

            def pp():
                if op == "eval_pdf":
                    _lib.check(lib.djb_eval_pp_batch(ctx._h, single._h, C.c_int64(n), C.byref(vi), C.byref(vo), at(gathered), C.c_int(5), C.byref(va), at(out_pdf), mem))
                else:
                    _lib.check(lib.djb_sample_pp_batch(ctx._h, single._h, C.c_int64(n), at(u1), at(u2), C.byref(vo), at(gathered), C.byref(va), C.byref(vb),
                                                       at(out_pdf), mem))
            state = {}

            def partition():
                with torch.cuda.stream(stream):
                    order = torch.sort(ids64).indices
                    state["order"] = order
                    if op == "eval_pdf":
                        torch.index_select(i, 1, order, out=si)
                    else:
                        torch.index_select(u1, 0, order, out=s1); torch.index_select(u2, 0, order, out=s2)
                    torch.index_select(o, 1, order, out=so)
                    state["bounds"] = [0] + torch.cumsum(torch.bincount(ids64, minlength=M), 0).cpu().tolist()        # the read-back of the sizes

            def part_calls():
                bounds = state["bounds"]
                for m in range(M):
                    lo, cnt = bounds[m], bounds[m + 1] - bounds[m]
                    if cnt:
                        one_call(members[m], params[m], cnt, lo, (si, so, s1, s2, sa, sb, spdf))

            def scatter():
                with torch.cuda.stream(stream):
                    order = state["order"]
                    out_a.index_copy_(1, order, sa); out_pdf.index_copy_(0, order, spdf)
                    if op != "eval_pdf":
                        out_b.index_copy_(1, order, sb)
            legs = {"set_uniform": lambda: set_call(uniform), "set_mixed": lambda: set_call(mixed)}
            if M <= ROWS_LDS:
                legs["set_global"] = lambda: set_call(uniform, True)
            legs["single"] = lambda: one_call(single, params[0], n, 0, plain)
            legs["gather_pp"] = lambda: (gather(), pp())
            legs["gather_pp.gather"] = gather
            legs["gather_pp.pp"] = pp
            if members:
                legs["partition"] = lambda: (partition(), part_calls(), scatter())
                legs["partition.partition"] = partition
                legs["partition.calls"] = part_calls
                legs["partition.scatter"] = scatter
            ms = {k: [] for k in legs}
            for r in range(args.warmup + args.repeats):
                for k, f in legs.items():                  # alternated: every round runs every leg once
                    ctx.timer_start(); f(); t = ctx.timer_stop_ms()
                    if r >= args.warmup:
                        ms[k].append(t)
            entry = {k: summarise(v, n, BYTES[op].get("set" if k.startswith("set") else k)) for k, v in ms.items()}

            def versus(a, b):
                return {"ratio_of_medians": round(entry[b]["ms_median"] / entry[a]["ms_median"], 3), "larger_spread": max(entry[a]["spread"], entry[b]["spread"])}
            entry["per_lane_rows_ms"] = round(entry["set_uniform"]["ms_median"] - entry["single"]["ms_median"], 4)
            entry["gather_pp_over_set_uniform"] = versus("set_uniform", "gather_pp")
            if members:
                entry["partition_over_set_mixed"] = versus("set_mixed", "partition")
            res["configs"][f"{kind} {op}"][str(M)] = entry
            print(kind, op, M, json.dumps(entry), flush=True)
            uniform.close(); mixed.close(); single.close()
            for b in members:
                b.close()
            del ids, ids64, gathered
            state.clear()
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
