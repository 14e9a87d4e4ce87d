#!/usr/bin/env python3
"""Cost of the inner fit's self-interpenetration term (csrc/fdc_collide.h), next to the same evaluation without it in this tree and in
another build of the library (--parent-lib: the commit before it).  The body is synth.make_body_mesh(10475): the grids' V and F are in
the output; the 23-joint layout, 64 and 1024 frames, capacity 8192 pairs per frame, parts by bone with a part never tested against
itself or its parent part.  Cases:
  parent     fdcap_opt_backward_fit2d, the build given as --parent-lib
  off        ... this tree, fdcap_opt_set_fit2d_collision never called
  on         ... with the term
  op         fdcap_collision_eval alone on the same frames' vertices, culled search, with the gradient
  op_search  ... with capacity 1: the penalty and the grouping shrink to their launches, what is left is refit + search
  op_leaf64  `op` with leaves of 64 faces (FDCAP_COLL_LEAF=64)
  op_every   `op` through the every-pair launch (64 frames only, 3 evaluations per stretch)
  fit_off / fit_on   one InnerFitOP.fitting() at 64 frames, L-BFGS, default stages: wall time
The split of `on` that the table states is by subtraction: the collision code = op, of which refit + search = op_search and penalty +
grouping = op - op_search; the full-mesh forward and backward it rides on = on - off - op.
Device events around stretches of 50 calls; every case runs in a process of its own, parent and tree alternated.  Nothing more is
started after a case that fails.  Writes profiles/collision_fit.json.
    python tools/collision_fit_timing.py --parent-lib PATH [--reps 2] [--out profiles/collision_fit.json]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fdcap_set_collision_mesh", "fdcap_collision_eval", "fdcap_debug_collision_tree", "fdcap_opt_set_fit2d_collision")
STRETCH, STRETCHES, WARMUP = 50, 10, 30
CAPACITY, SIGMA, WEIGHT = 8192, 0.5, 1.0


def child(mode, n):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import fdcap_amd  # noqa: F401
    from fdcap_amd import capi, ops, synth
    from fdcap_amd.innerfit import DEFAULT_INTRINSICS, InnerFitOP, collision_filter
    if mode == "parent":                                       # a build without the new entry points: bind what it exports
        for s in NEW_SYMBOLS:
            capi.SYMBOLS.pop(s, None)
    bm, part, parent = synth.make_body_mesh(10475, seed=0)
    vp = synth.make_vposer(seed=1)
    V, F = bm.num_verts, int(bm.faces.shape[0])
    rng = np.random.Generator(np.random.PCG64(5))
    clip = synth.make_clip(n, seed=2, num_outliers=0)
    rows = clip.body_params.astype(np.float32).copy()
    rows[:, 72:75] = np.array([0.1, -0.2, 3.5], np.float32)
    kp = np.concatenate([rng.uniform(100, 1100, (n, 23, 2)), rng.uniform(0.3, 1.0, (n, 23, 1))], -1).astype(np.float32)
    coll = dict(face_part=part, part_parent=parent, sigma=SIGMA, weights=(WEIGHT,) * 5, capacity=CAPACITY)
    out = {"mode": mode, "frames": n, "V": V, "F": F}
    us = []
    if mode.startswith("fit_"):
        op = InnerFitOP(bm, vp, n, optimizer="lbfgs", collision=dict(coll, weights=(0.0, 0.0, 0.0, 0.01, 1.0)) if mode == "fit_on" else None)
        op.fitting(rows, kp)                                   # (once to warm every allocation, then the timed one)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        op.fitting(rows, kp)
        torch.cuda.synchronize()
        out["wall_s"], out["rounds"] = time.perf_counter() - t0, op.rounds
        op.close()
    elif mode.startswith("op"):
        ctx = capi.Context(bm, vp)
        ctx.set_collision_mesh(bm.faces, part, collision_filter(part, parent))
        verts, _ = ops.body_forward_from_params(ctx, torch.tensor(rows, device="cuda"))
        cap = 1 if mode == "op_search" else CAPACITY
        count, loss, dv = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros_like(verts)
        prm = capi.CollisionParams(SIGMA, WEIGHT, cap, 1 if mode == "op_every" else 0)
        st = capi.current_stream()
        per = 3 if mode == "op_every" else STRETCH

        def stretch(k):
            for _ in range(k):
                capi.check(ctx.lib.fdcap_collision_eval(ctx.handle, capi.dptr(verts), n, prm, None, capi.dptr(count), capi.dptr(loss), capi.dptr(dv), st),
                           "fdcap_collision_eval")
        stretch(2 if mode == "op_every" else WARMUP)
        torch.cuda.synchronize()
        for _ in range(3 if mode == "op_every" else STRETCHES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            stretch(per)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / per)
        c = count.cpu().numpy()
        out["pairs_per_frame"] = {"min": int(c.min()), "median": float(np.median(c)), "max": int(c.max())}
        out["leaf"] = ctx.collision_tree()[0]
        ctx.close()
    else:
        op = InnerFitOP(bm, vp, n, iters_per_stage=0, collision=coll if mode == "on" else None)
        op.fitting(rows, kp)
        lib, h = op.ctx.lib, op.ctx.handle
        sg = capi.Fit2dStage(*DEFAULT_INTRINSICS, 100.0, 1.0, 4.78, 5.0, 4.78)
        st = capi.current_stream()

        def stretch(k):
            for _ in range(k):
                capi.check(lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 0, st), "fdcap_opt_backward_fit2d")
        stretch(WARMUP)
        torch.cuda.synchronize()
        for _ in range(STRETCHES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            stretch(STRETCH)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / STRETCH)
        op.close()
    out["us"] = us
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--parent-lib", required=False)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collision_fit.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.frames)
    plan = []
    for n in (64, 1024):
        plan += [(m, n) for m in ((["parent"] if a.parent_lib else []) + ["off", "on", "op", "op_search", "op_leaf64"])]
    once = [("op_every", 64), ("fit_off", 64), ("fit_on", 64)]
    runs = {}
    for rep in range(a.reps):
        for mode, n in plan + (once if rep == 0 else []):
            env = dict(os.environ)
            env.pop("FDCAP_COLL_LEAF", None)
            if mode == "op_leaf64":
                env["FDCAP_COLL_LEAF"] = "64"
            if mode == "parent":
                env["FDCAP_LIB"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--frames", str(n)], env=env, capture_output=True, text=True,
                               timeout=400)
            if p.returncode != 0:                              # nothing more is started after a failure
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{mode} at {n} frames ended with status {p.returncode}")
            r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            runs.setdefault((mode, n), []).append(r)
            what = f"median {statistics.median(r['us']):10.2f} us" if r["us"] else f"wall {r['wall_s']:.3f} s, rounds {r['rounds']}"
            print(f"{n:5d} frames {mode:10s} run {rep}: {what}", flush=True)
    table = []
    for (mode, n), rs in sorted(runs.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        row = {"mode": mode, "frames": n, "V": rs[0]["V"], "F": rs[0]["F"]}
        if rs[0]["us"]:
            med = [statistics.median(r["us"]) for r in rs]
            row.update(unit="us per call", median_of_runs=statistics.median(med), run_medians=med, min=min(min(r["us"]) for r in rs),
                       max=max(max(r["us"]) for r in rs))
        else:
            row.update(unit="s per fitting()", wall_s=[r["wall_s"] for r in rs], rounds=rs[0]["rounds"])
        for k in ("pairs_per_frame", "leaf"):
            if k in rs[0]:
                row[k] = rs[0][k]
        table.append(row)
    get = lambda m, n: next((t["median_of_runs"] for t in table if t["mode"] == m and t["frames"] == n and "median_of_runs" in t), None)
    split = []
    for n in (64, 1024):
        on, off, opv, srch = get("on", n), get("off", n), get("op", n), get("op_search", n)
        if None not in (on, off, opv, srch):
            split.append({"frames": n, "term_on_minus_off": on - off, "full_mesh_forward_and_backward": on - off - opv, "refit_and_search": srch,
                          "penalty_and_grouping": opv - srch})
    out = {"tool": "tools/collision_fit_timing.py", "body": "synth.make_body_mesh(10475, seed=0): synthetic, no real SMPL-X topology or segmentation",
           "capacity": CAPACITY, "sigma": SIGMA, "stretch": STRETCH, "stretches_per_run": STRETCHES, "runs_per_case": a.reps, "table": table,
           "split_by_subtraction": split}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(split, indent=1))


if __name__ == "__main__":
    main()
