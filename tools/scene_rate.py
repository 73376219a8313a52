#!/usr/bin/env python3
"""scene_rate.py -- rate of the scene call on one MI355X against the caller's own partition, written to profiles/scene/rate.json.

    python tools/scene_rate.py [--n HITS] [--repeats R] [--warmup W] [--materials 16,100] [--out FILE]

For M in {16, 100} materials PER KIND -- MERL and UTIA members from the synthetic tables of tools/merl_set_rate.py / utia_set_rate.py
(four contents, cycled), sgd and abc from the published rows (tools/model_set_rate.py) -- a scene of 4 M slots (slot = kind * M + local)
and n dense device-resident hits (i, o from gen_directions with z > 0: all above the horizon) it times evalp:
  scene_random      the scene call, kinds and materials drawn per hit
  scene_runs4096    the scene call, the kind constant over runs of 4 096 hits (materials drawn per hit)
  scene_sorted      the scene call, ids sorted (kind-major)
  one_<kind>        the scene call on a scene of that ONE kind (M slots, ids drawn) ...
  set_<kind>        ... against that member set's own call on the same ids: the difference is what the partition and the indirection cost
  caller            the caller's route on the same build: a torch partition by kind (stable sort of the kinds, gathers of ids, i, o; the
                    four sub-batch sizes read back to the host), the four member-set calls on the sub-batches, a scatter of the results.
                    Timed as a whole; caller_partition / caller_calls / caller_scatter are its parts, timed inside the same rounds
Method (the measuring guide's): one process, everything resident in HBM, W warm-up rounds, then R rounds in which the legs run
ALTERNATELY, each leg between two HIP events on the stream the context and torch share.  Median, min, max and spread = (max - min) /
median per leg.  Bytes per hit are COUNTED from the signatures, not measured: the streams move 40 B (id 4, i 12, o 12, out 12); the
partition adds two id reads, one slot read and one 4 B list write (16 B), each evaluated hit one list read and one more id read (8 B).
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
KINDS = ("merl", "utia", "sgd", "abc")
BYTES = {"scene": 40 + 16 + 8, "set": 40}


def summarise(ms, n, nbytes=None):
    med = statistics.median(ms)
    r = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4),
         "timed_calls": len(ms), "Ghits_per_s": round(n / med / 1e6, 3)}
    if nbytes:
        r.update({"bytes_per_hit_counted": nbytes, "algorithmic_GBps": round(n * nbytes / med / 1e6, 1)})
    return r


def utia_tables(synth):
    smooth = synth.utia_table_smooth()
    rev = np.ascontiguousarray(smooth.reshape(3, 6, 48, 6, 48)[:, :, ::-1, :, ::-1]).reshape(-1)
    return [smooth, rev] + [np.random.default_rng(s).uniform(0.0, 120.0, synth.UTIA_N) for s in (11, 12)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--materials", default="16,100")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene", "rate.json"))
    args = ap.parse_args()
    import torch
    from dj_brdf_amd import _lib, djb, param_tables, synth
    lib = _lib.load()
    ctx = djb.default_context(0)
    dev, n = "cuda:0", args.n
    i = djb.gen_directions(n, synth.SEED_I, ctx=ctx); o = djb.gen_directions(n, synth.SEED_O, ctx=ctx)
    i[2].abs_(); o[2].abs_()
    out = torch.empty((3, n), dtype=torch.float32, device=dev)
    mem = C.c_int(_lib.MEM_DEVICE)

    def view(t, cols=None):
        """the SoA view of a [3, cols] tensor"""
        cols = t.shape[1] if cols is None else cols
        v = _lib.Vec3View()
        v.x, v.y, v.z, v.stride = t.data_ptr(), t.data_ptr() + 4 * cols, t.data_ptr() + 8 * cols, 1
        return v
    merl_src = [djb.merl.from_table(synth.merl_table(*synth.material_recipe(m)), ctx=ctx) for m in range(4)]
    utia_src = [djb.utia.from_table(t, ctx=ctx) for t in utia_tables(synth)]
    rows = {"sgd": np.array([param_tables.sgd_params(name) for name in synth.MERL_NAMES], np.float64),
            "abc": np.array([param_tables.abc_params(name) for name in synth.MERL_NAMES], np.float64)}
    res = {"n": n, "call": "evalp", "timing": "HIP events around each leg; legs alternated inside every round", "warmup_rounds": args.warmup,
           "bytes_per_hit": "counted from the signatures, not measured", "materials_per_kind": {}}
    vi, vo, vout = view(i), view(o), view(out)
    for M in [int(x) for x in args.materials.split(",")]:
        sets = {"merl": djb.merl_set([merl_src[m % 4] for m in range(M)], ctx=ctx), "utia": djb.utia_set([utia_src[m % 4] for m in range(M)], ctx=ctx),
                "sgd": djb.model_set.from_rows("sgd", rows["sgd"][np.arange(M) % 100], ctx=ctx),
                "abc": djb.model_set.from_rows("abc", rows["abc"][np.arange(M) % 100], ctx=ctx)}
        whole = djb.scene(slots=[(k, m) for k in KINDS for m in range(M)], ctx=ctx, **sets)
        ones = {k: djb.scene(slots=[(k, m) for m in range(M)], ctx=ctx, **{k: sets[k]}) for k in KINDS}
        g = torch.Generator(device=dev); g.manual_seed(4321 + M)
        local = torch.randint(0, M, (n,), generator=g, device=dev, dtype=torch.int32)
        ids_random = (torch.randint(0, 4, (n,), generator=g, device=dev, dtype=torch.int32) * M + local).contiguous()
        runs = torch.randint(0, 4, ((n + 4095) // 4096,), generator=g, device=dev, dtype=torch.int32).repeat_interleave(4096)[:n]
        ids_runs = (runs * M + local).contiguous()
        ids_sorted = torch.sort(ids_random).values.contiguous()
        del runs

        def scene_eval(s, which):
            _lib.check(lib.djb_scene_eval_batch(ctx._h, s._h, C.c_int64(n), C.c_void_p(which.data_ptr()), C.byref(vi), C.byref(vo), C.c_int(1),
                                                C.byref(vout), mem))

        def set_eval(kind, cnt, which, a, b, c):
            fn = getattr(lib, {"merl": "djb_merl_set_eval_batch", "utia": "djb_utia_set_eval_batch"}.get(kind, "djb_model_set_eval_batch"))
            _lib.check(fn(ctx._h, sets[kind]._h, C.c_int64(cnt), C.c_void_p(which.data_ptr()), C.byref(a), C.byref(b), C.c_int(1), C.byref(c), mem))
        parts = {"caller_partition": [], "caller_calls": [], "caller_scatter": []}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

        def caller():
            """what a renderer does today: split by kind, gather, four set calls, scatter back"""
            ev[0].record()
            kind = torch.div(ids_random, M, rounding_mode="floor")
            order = torch.sort(kind, stable=True).indices
            counts = torch.bincount(kind, minlength=4).cpu().tolist()          # the host needs the sub-batch sizes
            sub_ids = (ids_random[order] % M).to(torch.int32).contiguous()
            sub_i, sub_o = i[:, order].contiguous(), o[:, order].contiguous()
            sub_out = torch.empty_like(sub_i)
            ev[1].record()
            lo = 0
            for q, k in enumerate(KINDS):
                cnt = counts[q]
                if cnt:
                    a, b, c = _lib.Vec3View(), _lib.Vec3View(), _lib.Vec3View()
                    for v, t in ((a, sub_i), (b, sub_o), (c, sub_out)):
                        base = t.data_ptr() + 4 * lo
                        v.x, v.y, v.z, v.stride = base, base + 4 * n, base + 8 * n, 1
                    set_eval(k, cnt, sub_ids[lo:], a, b, c)
                lo += cnt
            ev[2].record()
            out[:, order] = sub_out
            ev[3].record()
        legs = {"scene_random": lambda: scene_eval(whole, ids_random), "scene_runs4096": lambda: scene_eval(whole, ids_runs),
                "scene_sorted": lambda: scene_eval(whole, ids_sorted)}
        for k in KINDS:
            legs["one_" + k] = (lambda k=k: scene_eval(ones[k], local))
            legs["set_" + k] = (lambda k=k: set_eval(k, n, local, vi, vo, vout))
        legs["caller"] = caller
        ms = {k: [] for k in legs}
        for r in range(args.warmup + args.repeats):
            for k, f in legs.items():                      # alternated: every round runs every leg once
                ctx.timer_start(); f(); t = ctx.timer_stop_ms()
                if r >= args.warmup:
                    ms[k].append(t)
                    if k == "caller":
                        for name, a in zip(parts, range(3)):
                            parts[name].append(ev[a].elapsed_time(ev[a + 1]))
        entry = {k: summarise(v, n, BYTES["scene" if k.startswith(("scene", "one")) else "set"] if k != "caller" else None) for k, v in ms.items()}
        entry.update({k: summarise(v, n) for k, v in parts.items()})
        res["materials_per_kind"][str(M)] = entry
        print(M, json.dumps(entry), flush=True)
        for s in [whole] + list(ones.values()) + list(sets.values()):
            s.close()
        del ids_random, ids_runs, ids_sorted, local
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
