#!/usr/bin/env python3
"""Cost of one objective evaluation, and of one L-BFGS round, of the inner fit with free expression coefficients, next to the same
evaluation without them in this tree and in another build of the library (--parent-lib: the commit before).  tools/face_fit_timing.py's
protocol on its case (d) -- 67 + 51 mapped keypoints on the V = 10 475 synthetic body -- at 64 and 1024 frames, the set's blend products
in the kernel (k) and as panel products around it (p), FDCAP_KP_BLEND pinned either way:
  parent     the build given as --parent-lib
  off        this tree, fdcap_opt_set_expression never called
  jaw        fdcap_opt_set_jaw                                   (the rows the expression's are read next to)
  expr       fdcap_opt_set_expression
  expr_jaw   both
and `lbfgs_*`: 40 rounds of fdcap_opt_fit2d_lbfgs on (dk) at 64 frames with the jaw (81 unknowns), the coefficients (88) and both (91).
Device events around stretches of 50 fdcap_opt_backward_fit2d calls; every case runs in a process of its own, parent and tree
alternated, two runs.  Nothing more is started after a case that fails.  Writes profiles/expression_fit.json.
    python tools/expression_fit_timing.py --parent-lib PATH [--reps 2] [--out profiles/expression_fit.json]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fdcap_opt_set_expression", "fdcap_opt_get_expression", "fdcap_opt_set_expression_prior")
STRETCH, STRETCHES, WARMUP, LBFGS_ROUNDS = 50, 10, 30, 40
LAUNCHES = {"k": 5, "p": 7}                                  # per evaluation (tools/keypoint_fit_timing.py); the expression adds none


def child(mode, case, n):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import fdcap_amd  # noqa: F401
    from fdcap_amd import capi, synth
    from fdcap_amd.innerfit import DEFAULT_INTRINSICS, DEFAULT_LBFGS, OPENPOSE_BODY25, OPENPOSE_LHAND, OPENPOSE_RHAND, InnerFitOP, KeypointMap
    if mode == "parent":                                     # a build without the new entry points: bind what it exports
        for s in NEW_SYMBOLS:
            capi.SYMBOLS.pop(s, None)
    bm, vp = synth.make_body_model(seed=0), synth.make_vposer(seed=1)
    V = bm.v_template.shape[0]
    rng = np.random.Generator(np.random.PCG64(5))
    idx = list(OPENPOSE_BODY25 + OPENPOSE_LHAND + OPENPOSE_RHAND) + list(range(76, 127))
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
    jaw0 = torch.tensor(0.1 * rng.standard_normal((n, 3)).astype(np.float32), device="cuda")
    psi0 = torch.tensor(rng.standard_normal((n, 10)).astype(np.float32), device="cuda")

    def free():                                              # (an L-BFGS run moves them: every run starts from the same point)
        if "jaw" in mode:
            capi.check(lib.fdcap_opt_set_jaw(h, capi.dptr(jaw0), st), "fdcap_opt_set_jaw")
            ex = capi.Fit2dExtra()
            ex.w_jaw[0], ex.w_jaw[1], ex.w_jaw[2] = 47.8, 478.0, 478.0
            capi.check(lib.fdcap_opt_set_fit2d_extra(h, ctypes.byref(ex)), "fdcap_opt_set_fit2d_extra")
        if "expr" in mode:
            capi.check(lib.fdcap_opt_set_expression(h, capi.dptr(psi0), st), "fdcap_opt_set_expression")
            capi.check(lib.fdcap_opt_set_expression_prior(h, 5.0), "fdcap_opt_set_expression_prior")
    free()
    us = []
    if mode.startswith("lbfgs"):
        q = dict(DEFAULT_LBFGS, max_iter=1000, max_steps=1000)
        cf = capi.LbfgsConfig(capi.XDIM, q["history"], q["max_iter"], q["max_eval"], q["max_steps"], q["max_ls"], q["lr"], q["tolerance_grad"],
                              q["tolerance_change"], q["ftol"], q["gtol"])
        x0 = op._rows_x.clone()
        for k in range(STRETCHES + 2):
            op._rows_x.copy_(x0)
            free()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expression_fit.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.frames)
    plan = []
    for n in (64, 1024):
        for case in ("dk", "dp"):
            plan += [(m, case, n) for m in ((["parent"] if a.parent_lib else []) + ["off", "jaw", "expr", "expr_jaw"])]
    plan += [(m, "dk", 64) for m in ("lbfgs_jaw", "lbfgs_expr", "lbfgs_expr_jaw")]
    runs = {}
    for rep in range(a.reps):
        for mode, case, n in plan:
            env = dict(os.environ)
            env["FDCAP_KP_BLEND"] = "kernel" if case[1] == "k" else "panel"
            if mode == "parent":
                env["FDCAP_LIB"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, case, "--frames", str(n)], env=env, capture_output=True,
                               text=True, timeout=300)
            if p.returncode != 0:                            # nothing more is started after a failure
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{mode} {case} at {n} frames ended with status {p.returncode}")
            r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            runs.setdefault((mode, case, n), []).append(r)
            print(f"{n:5d} frames {case} {mode:14s} run {rep}: median {statistics.median(r['us']):8.2f} us", flush=True)
    table = []
    for (mode, case, n), rs in sorted(runs.items(), key=lambda kv: (kv[0][2], kv[0][1], kv[0][0])):
        med = [statistics.median(r["us"]) for r in rs]
        table.append({"mode": mode, "case": case, "frames": n, "keypoints": rs[0]["keypoints"],
                      "unit": "us per round (evaluation + advance)" if mode.startswith("lbfgs") else "us per evaluation",
                      "launches_per_eval": LAUNCHES[case[1]] + int(mode.startswith("lbfgs")),
                      "unknowns_per_frame": 78 + (3 if "jaw" in mode else 0) + (10 if "expr" in mode else 0),
                      "median_of_runs": statistics.median(med), "run_medians": med, "min": min(min(r["us"]) for r in rs), "max": max(max(r["us"]) for r in rs)})
    out = {"tool": "tools/expression_fit_timing.py", "body_vertices": 10475, "stretch": STRETCH, "stretches_per_run": STRETCHES, "runs_per_case": a.reps,
           "lbfgs_rounds": LBFGS_ROUNDS, "table": table}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for t in table:
        print(f"{t['frames']:5d} frames {t['case']} {t['mode']:14s}: {t['median_of_runs']:8.2f} {t['unit']} (runs {', '.join(f'{m:.2f}' for m in t['run_medians'])}; "
              f"stretches {t['min']:.2f} .. {t['max']:.2f}; {t['launches_per_eval']} launches)")


if __name__ == "__main__":
    main()
