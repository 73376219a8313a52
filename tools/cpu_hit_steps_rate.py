#!/usr/bin/env python3
"""cpu_hit_steps_rate.py -- time of the per-hit calls of a CPU context, this tree's library against another build of it (the parent
commit's), written to profiles/host_hit_steps/cpu_rate.json.

    python tools/cpu_hit_steps_rate.py --other-lib PATH [--n HITS] [--rounds R] [--calls K] [--materials M] [--out FILE]

Twelve calls on Context("cpu"), numpy arrays, n = 2^20 hits above the horizon: eval, the sampling step and the light sample of a MERL set,
an sgd model set and a scene of all four kinds (M materials per kind, ids drawn per hit); the single-material proxy pair (a MERL table
under a ggx lobe); the UTIA set's eval.  Each library runs in child processes of its own (DJB_LIB_PATH), R per side, ALTERNATED; a child
makes 1 warm-up round and K timed rounds in which the legs run one after the other.  Per leg and side: median, min, max and spread =
(max - min) / median over the R * K timed calls.  Rule: the tree's median does not exceed the other's by more than the larger of the two
spreads -- it bounds a regression at the spread and resolves nothing below it.  Needs no GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child(n, M, calls):
    import scene_rate
    from dj_brdf_amd import djb, param_tables, synth
    ctx = djb.cpu_context()
    i, o = synth.directions_aos(n, synth.SEED_I), synth.directions_aos(n, synth.SEED_O)
    i[:, 2] = np.abs(i[:, 2]); o[:, 2] = np.abs(o[:, 2])
    u1, u2 = synth.uniforms(n, synth.SEED_U1), synth.uniforms(n, synth.SEED_U2)
    P = djb.microfacet.params
    params = [P.isotropic(0.08 + 0.5 * m / max(M - 1, 1)) for m in range(M)]
    merls = [djb.merl.from_table(synth.merl_table(*synth.material_recipe(m)), ctx=ctx) for m in range(min(M, 4))]
    utias = [djb.utia.from_table(t, ctx=ctx) for t in scene_rate.utia_tables(synth)]
    rows = {k: np.array([getattr(param_tables, k + "_params")(name) for name in synth.MERL_NAMES], np.float64)[np.arange(M) % 100] for k in ("sgd", "abc")}
    sets = {"merl": djb.merl_set([merls[m % len(merls)] for m in range(M)], params, ctx=ctx),
            "utia": djb.utia_set([utias[m % 4] for m in range(M)], ctx=ctx),
            "sgd": djb.model_set.from_rows("sgd", rows["sgd"], ctx=ctx), "abc": djb.model_set.from_rows("abc", rows["abc"], ctx=ctx)}
    sets["utia"].set_proxy_params(params)
    sets["sgd"].fit_proxy(90, True); sets["abc"].fit_proxy(90, True)
    whole = djb.scene(slots=[(k, m) for k in ("merl", "utia", "sgd", "abc") for m in range(M)], ctx=ctx, **sets)
    lobe = djb.ggx(ctx=ctx)
    rng = np.random.default_rng(8765 + M)
    ids = rng.integers(0, M, n, dtype=np.int32)
    sids = (rng.integers(0, 4, n, dtype=np.int32) * M + ids).astype(np.int32)
    legs = {
        "merl_set_eval": lambda: sets["merl"].evalp(ids, i, o),
        "merl_set_sampling": lambda: sets["merl"].evalp_is_proxy(lobe, ids, u1, u2, o),
        "merl_set_light": lambda: sets["merl"].evalp_pdf_proxy(lobe, ids, i, o),
        "model_set_eval": lambda: sets["sgd"].evalp(ids, i, o),
        "model_set_sampling": lambda: sets["sgd"].evalp_is_proxy(ids, u1, u2, o),
        "model_set_light": lambda: sets["sgd"].evalp_pdf_proxy(ids, i, o),
        "scene_eval": lambda: whole.evalp(sids, i, o),
        "scene_sampling": lambda: whole.evalp_is_proxy(lobe, sids, u1, u2, o),
        "scene_light": lambda: whole.evalp_pdf_proxy(lobe, sids, i, o),
        "single_sampling": lambda: merls[0].evalp_is_proxy(lobe, u1, u2, o, None, params[0]),
        "single_light": lambda: merls[0].evalp_pdf_proxy(lobe, i, o, None, params[0]),
        "utia_set_eval": lambda: sets["utia"].evalp(ids, i, o),
    }
    ms = {k: [] for k in legs}
    for r in range(1 + calls):
        for k, f in legs.items():
            t0 = time.perf_counter(); f(); t = (time.perf_counter() - t0) * 1e3
            if r:
                ms[k].append(t)
    print("LEGS " + json.dumps(ms), flush=True)


def summarise(ms):
    med = statistics.median(ms)
    return {"ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "spread": round((max(ms) - min(ms)) / med, 4),
            "timed_calls": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--materials", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host_hit_steps", "cpu_rate.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.n, args.materials, args.calls)
    if not args.other_lib:
        ap.error("--other-lib: the library to compare with (a build of the parent commit)")
    sides = {"tree": None, "other": os.path.abspath(args.other_lib)}
    ms = {s: {} for s in sides}
    for r in range(args.rounds):
        for side, path in sides.items():
            env = dict(os.environ)
            env.pop("DJB_LIB_PATH", None)
            if path:
                env["DJB_LIB_PATH"] = path
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--calls", str(args.calls),
                                  "--materials", str(args.materials)], env=env, check=True, capture_output=True, text=True).stdout
            got = json.loads([l for l in out.splitlines() if l.startswith("LEGS ")][-1][5:])
            for k, v in got.items():
                ms[side].setdefault(k, []).extend(v)
            print(f"round {r} {side}: " + ", ".join(f"{k} {statistics.median(v):.1f}" for k, v in got.items()), flush=True)
    legs, outside = {}, []
    for k in ms["tree"]:
        t, p = summarise(ms["tree"][k]), summarise(ms["other"][k])
        bound = max(t["spread"], p["spread"])
        over = t["ms_median"] / p["ms_median"] - 1.0
        legs[k] = {"tree": t, "other": p, "tree_over_other": round(over, 4), "bound": bound, "within_bound": over <= bound}
        if over > bound:
            outside.append(k)
    res = {"what": "wall time per call on Context('cpu'), numpy arrays; this tree's library against --other-lib, child processes alternated",
           "command": "python tools/cpu_hit_steps_rate.py --other-lib <library built from the parent commit>" +
                      f" --n {args.n} --rounds {args.rounds} --calls {args.calls} --materials {args.materials}",
           "rule": "tree median <= other median * (1 + max(tree spread, other spread)); spread = (max - min) / median",
           "n": args.n, "materials_per_kind": args.materials, "cpus": os.cpu_count(), "legs": legs, "legs_outside_bound": outside}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
