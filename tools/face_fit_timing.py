#!/usr/bin/env python3
"""Cost of one objective evaluation of the inner fit with a free jaw and / or the bending prior, next to the same evaluation without
them in this tree and in another build of the library (--parent-lib: the commit before both).  Cases (c) and (d) of
tools/keypoint_fit_timing.py -- 67 mapped keypoints, and 67 + 51 face landmarks -- on the V = 10 475 synthetic body at 64 and 1024
frames, the set's blend products in the kernel (k) and as panel products around it (p), FDCAP_KP_BLEND pinned either way:
  parent   the build given as --parent-lib                        (ck cp dk dp)
  off      this tree, neither entry point called                  (ck cp dk dp)
  jaw      fdcap_opt_set_jaw                                       (dk dp: the map with a face)
  bend     fdcap_opt_set_fit2d_extra with the four default terms  (dk dp)
  both                                                             (dk dp)
and `lbfgs`: 40 rounds of fdcap_opt_fit2d_lbfgs on (dk) at 64 frames, parent and off -- the advance kernel's share of a round.
Device events around stretches of fdcap_opt_backward_fit2d calls; every case runs in a process of its own, the cases alternated so
that drift of the machine falls on all alike.  Nothing more is started after a case that fails.  Writes profiles/face_fit.json.
    python tools/face_fit_timing.py --parent-lib PATH [--reps 2] [--out profiles/face_fit.json]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fdcap_opt_set_fit2d_extra", "fdcap_opt_set_jaw", "fdcap_opt_get_jaw", "fdcap_opt_fit2d_lbfgs_rolled_back")
STRETCH, STRETCHES, WARMUP, LBFGS_ROUNDS = 50, 10, 30, 40
LAUNCHES = {"k": 5, "p": 7}                                  # per evaluation without the feature (tools/keypoint_fit_timing.py)


def child(mode, case, n):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import fdcap_amd  # noqa: F401
    from fdcap_amd import capi, synth
    from fdcap_amd.innerfit import (DEFAULT_BEND_RATIO, DEFAULT_BEND_TERMS, DEFAULT_INTRINSICS, DEFAULT_LBFGS, OPENPOSE_BODY25, OPENPOSE_LHAND,
                                    OPENPOSE_RHAND, InnerFitOP, KeypointMap)
    if mode in ("parent", "lbfgs_parent"):                   # a build without the new entry points: bind what it exports
        for s in NEW_SYMBOLS:
            capi.SYMBOLS.pop(s, None)
    bm, vp = synth.make_body_model(seed=0), synth.make_vposer(seed=1)
    V = bm.v_template.shape[0]
    rng = np.random.Generator(np.random.PCG64(5))
    idx = list(OPENPOSE_BODY25 + OPENPOSE_LHAND + OPENPOSE_RHAND) + (list(range(76, 127)) if case[0] == "d" else [])
    ids = rng.permutation(V)
    kmap = KeypointMap.from_smplx_indices(idx, ids[:21], ids[21:21 + 153].reshape(51, 3), rng.dirichlet((1.0, 1.0, 1.0), 51))
    nkp = len(kmap)
    clip = synth.make_clip(n, seed=2, num_outliers=0)
    rows = clip.body_params.astype(np.float32).copy()
    rows[:, 72:75] = np.array([0.1, -0.2, 3.5], np.float32)
    kp = np.concatenate([rng.uniform(100, 1100, (n, nkp, 2)), rng.uniform(0.3, 1.0, (n, nkp, 1))], -1).astype(np.float32)
    op = InnerFitOP(bm, vp, n, iters_per_stage=0, keypoint_map=kmap)
    op.fitting(rows, kp)
    lib, h = op.ctx.lib, op.ctx.handle
    sg = capi.Fit2dStage(*DEFAULT_INTRINSICS, 100.0, 1.0, 4.78, 5.0, 4.78)
    st = capi.current_stream()
    if mode in ("jaw", "both"):
        jaw = torch.tensor(0.1 * rng.standard_normal((n, 3)).astype(np.float32), device="cuda")
        capi.check(lib.fdcap_opt_set_jaw(h, capi.dptr(jaw), st), "fdcap_opt_set_jaw")
    if mode in ("jaw", "bend", "both"):
        ex = capi.Fit2dExtra()
        ex.w_jaw[0], ex.w_jaw[1], ex.w_jaw[2] = 47.8, 478.0, 478.0
        if mode != "jaw":
            ex.w_bend, ex.n_bend = DEFAULT_BEND_RATIO * 4.78, len(DEFAULT_BEND_TERMS)
            for t, (j, a, s) in enumerate(DEFAULT_BEND_TERMS):
                ex.joint[t], ex.axis[t], ex.sign[t] = j, a, s
        capi.check(lib.fdcap_opt_set_fit2d_extra(h, ctypes.byref(ex)), "fdcap_opt_set_fit2d_extra")
    us = []
    if mode.startswith("lbfgs"):
        q = dict(DEFAULT_LBFGS, max_iter=1000, max_steps=1000)
        cf = capi.LbfgsConfig(capi.XDIM, q["history"], q["max_iter"], q["max_eval"], q["max_steps"], q["max_ls"], q["lr"], q["tolerance_grad"],
                              q["tolerance_change"], q["ftol"], q["gtol"])
        x0 = op._rows_x.clone()
        for k in range(STRETCHES + 2):
            op._rows_x.copy_(x0)
            rounds = ctypes.c_int32(0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            capi.check(lib.fdcap_opt_fit2d_lbfgs(h, ctypes.byref(sg), ctypes.byref(cf), LBFGS_ROUNDS, ctypes.byref(rounds), st), "fdcap_opt_fit2d_lbfgs")
            e1.record()
            e1.synchronize()
            if k >= 2:
                us.append(e0.elapsed_time(e1) * 1e3 / max(1, rounds.value))
    else:
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
    print("RESULT " + json.dumps({"mode": mode, "case": case, "frames": n, "keypoints": nkp, "us": us}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--parent-lib", required=False)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_fit.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.frames)
    plan = []
    for n in (64, 1024):
        for case in ("ck", "cp", "dk", "dp"):
            plan += [(m, case, n) for m in ((["parent"] if a.parent_lib else []) + ["off"])]
            if case[0] == "d":
                plan += [(m, case, n) for m in ("jaw", "bend", "both")]
    plan += [(m, "dk", 64) for m in ((["lbfgs_parent"] if a.parent_lib else []) + ["lbfgs_off"])]
    runs = {}
    for rep in range(a.reps):
        for mode, case, n in plan:
            env = dict(os.environ)
            env["FDCAP_KP_BLEND"] = "kernel" if case[1] == "k" else "panel"
            if mode.endswith("parent"):
                env["FDCAP_LIB"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, case, "--frames", str(n)], env=env, capture_output=True,
                               text=True, timeout=300)
            if p.returncode != 0:                            # nothing more is started after a failure
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{mode} {case} at {n} frames ended with status {p.returncode}")
            r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            runs.setdefault((mode, case, n), []).append(r)
            print(f"{n:5d} frames {case} {mode:12s} run {rep}: median {statistics.median(r['us']):8.2f} us", flush=True)
    table = []
    for (mode, case, n), rs in sorted(runs.items(), key=lambda kv: (kv[0][2], kv[0][1], kv[0][0])):
        med = [statistics.median(r["us"]) for r in rs]
        extra = int(mode in ("bend", "both"))                # the bending prior's launch; the jaw adds none
        table.append({"mode": mode, "case": case, "frames": n, "keypoints": rs[0]["keypoints"],
                      "unit": "us per round (evaluation + advance)" if mode.startswith("lbfgs") else "us per evaluation",
                      "launches_per_eval": LAUNCHES[case[1]] + extra + int(mode.startswith("lbfgs")),
                      "dPF_route": "one launch between the data term (or its blend backward) and the pose backward adds the terms to dPF" if extra else None,
                      "median_of_runs": statistics.median(med), "run_medians": med, "min": min(min(r["us"]) for r in rs), "max": max(max(r["us"]) for r in rs)})
    out = {"tool": "tools/face_fit_timing.py", "body_vertices": 10475, "stretch": STRETCH, "stretches_per_run": STRETCHES, "runs_per_case": a.reps,
           "lbfgs_rounds": LBFGS_ROUNDS, "table": table}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for t in table:
        print(f"{t['frames']:5d} frames {t['case']} {t['mode']:12s}: {t['median_of_runs']:8.2f} {t['unit']} (runs {', '.join(f'{m:.2f}' for m in t['run_medians'])}; "
              f"stretches {t['min']:.2f} .. {t['max']:.2f}; {t['launches_per_eval']} launches)")


if __name__ == "__main__":
    main()
