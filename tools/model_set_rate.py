#!/usr/bin/env python3
"""model_set_rate.py -- rate of the SGD / ABC model-set call on one MI355X, written to profiles/model_set/rate.json.

    python tools/model_set_rate.py [--n HITS] [--repeats R] [--warmup W] [--materials 1,16,100,4096] [--kinds sgd,abc] [--out FILE]

For each kind and M in {1, 16, 100, 4096} resident rows (the 100 published rows, cycled over the set) and n dense device-resident hits
(i, o from gen_directions with z > 0: all above the horizon; ids uniform over [0, M)) it times evalp:
  set_random    the set call, ids as drawn                      (40 B per hit, counted from the signature)
  set_sorted    the set call, ids sorted (hits of a material are contiguous)
  set_global    the set call with DJB_OPT_MODEL_SET_ROWS_GLOBAL, ids as drawn -- only where M fits the kernel's LDS budget (ROWS_LDS below:
                rows_lds() of djb_kernels_model_set.hip), i.e. where set_random reads its rows from LDS
  partitioned   M calls of djb_evalp_batch on the slices of the sorted batch: the floor a caller-side partition could reach; the
                partition itself is not timed
  single        M = 1 only, instead of `partitioned`: the plain djb_evalp_batch on the whole batch (36 B per hit)
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
BYTES = {"set": 40, "single": 36}
ROWS_LDS = {"sgd": 101, "abc": 213}


def summarise(ms, n, nbytes):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4),
            "timed_calls": len(ms), "Ghits_per_s": round(n / med / 1e6, 3), "bytes_per_hit": nbytes, "algorithmic_GBps": round(n * nbytes / med / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--materials", default="1,16,100,4096")
    ap.add_argument("--kinds", default="sgd,abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_set", "rate.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from dj_brdf_amd import _lib, djb, param_tables, synth
    lib = _lib.load()
    ctx = djb.default_context(0)
    dev, n = "cuda:0", args.n
    i = djb.gen_directions(n, synth.SEED_I, ctx=ctx); o = djb.gen_directions(n, synth.SEED_O, ctx=ctx)
    i[2].abs_(); o[2].abs_()
    out = torch.empty((3, n), dtype=torch.float32, device=dev)
    mem = C.c_int(_lib.MEM_DEVICE)

    def view(t, lo=0):
        """the SoA view of the units from lo on of a [3, n] tensor"""
        v = _lib.Vec3View()
        base = t.data_ptr() + 4 * lo
        v.x, v.y, v.z, v.stride = base, base + 4 * n, base + 8 * n, 1
        return v
    res = {"n": n, "call": "evalp", "timing": "HIP events around each leg; legs alternated inside every round", "warmup_rounds": args.warmup,
           "rows_lds": ROWS_LDS, "kinds": {}}
    for kind in args.kinds.split(","):
        look = param_tables.sgd_params if kind == "sgd" else param_tables.abc_params
        rows = np.array([look(name) for name in synth.MERL_NAMES], np.float64)
        cls = djb.sgd if kind == "sgd" else djb.abc
        members = [cls.from_params(r, ctx=ctx) for r in rows]
        res["kinds"][kind] = {}
        for M in [int(x) for x in args.materials.split(",")]:
            mset = djb.model_set.from_rows(kind, rows[np.arange(M) % len(rows)], ctx=ctx)
            g = torch.Generator(device=dev); g.manual_seed(1234 + M)
            ids = torch.randint(0, M, (n,), generator=g, device=dev, dtype=torch.int32)
            ids_sorted = torch.sort(ids).values.contiguous()
            bounds = torch.searchsorted(ids_sorted, torch.arange(M + 1, device=dev, dtype=torch.int32)).cpu().tolist()
            vi, vo, vout = view(i), view(o), view(out)

            def set_eval(which, rows_global=False):
                if rows_global:
                    djb.set_model_set_rows_global(ctx, True)
                _lib.check(lib.djb_model_set_eval_batch(ctx._h, mset._h, C.c_int64(n), C.c_void_p(which.data_ptr()), C.byref(vi), C.byref(vo), C.c_int(1),
                                                        C.byref(vout), mem))
                if rows_global:
                    djb.set_model_set_rows_global(ctx, False)

            def part_eval():
                for m in range(M):
                    lo, cnt = bounds[m], bounds[m + 1] - bounds[m]
                    if cnt:
                        a, b, c = view(i, lo), view(o, lo), view(out, lo)
                        _lib.check(lib.djb_evalp_batch(ctx._h, members[m % len(members)]._h, C.c_int64(cnt), C.byref(a), C.byref(b), None, C.byref(c), mem))
            legs = {"set_random": lambda: set_eval(ids), "set_sorted": lambda: set_eval(ids_sorted)}
            if M <= ROWS_LDS[kind]:
                legs["set_global"] = lambda: set_eval(ids, True)
            legs["single" if M == 1 else "partitioned"] = part_eval
            ms = {k: [] for k in legs}
            for r in range(args.warmup + args.repeats):
                for k, f in legs.items():                  # alternated: every round runs every leg once
                    ctx.timer_start(); f(); t = ctx.timer_stop_ms()
                    if r >= args.warmup:
                        ms[k].append(t)
            entry = {k: summarise(v, n, BYTES["set" if k.startswith("set") else "single"]) for k, v in ms.items()}
            res["kinds"][kind][str(M)] = entry
            print(kind, M, json.dumps(entry), flush=True)
            mset.close()
            del ids, ids_sorted
            torch.cuda.empty_cache()
        for b in members:
            b.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
