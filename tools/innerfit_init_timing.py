#!/usr/bin/env python3
"""Cost of the inner fit's start from keypoints alone (csrc/fdc_fit2d_init.h), on the 23-joint layout of the V = 10 475 synthetic body:
  camera_eval    us per fdcap_opt_backward_fit2d_camera evaluation (one launch; the set-up's forward is outside the stretches)
  full_eval      us per fdcap_opt_backward_fit2d evaluation, the full objective, from the same run
  camera_round   us per round of fdcap_opt_fit2d_camera_lbfgs (evaluation + advance, its polling included)
at 64 and 1024 frames, and at 64 frames
  fit_init       ms of InnerFitOP(init={}, optimizer="lbfgs").fitting(None, keypoints): guess, camera stages, the twins' problems, five
                 stages over n + m problems, frame loss, select
  fit_both       the same with orientations="both": m = n, every frame gets its twin
  fit_stages     ms of InnerFitOP(optimizer="lbfgs").fitting(rows, keypoints) from the rows the camera stage left: the five stages alone
The protocol of tools/face_fit_timing.py: device events around stretches of 50 evaluations, every case in a process of its own, the
cases alternated, two runs; nothing more is started after a case that fails.  Writes profiles/innerfit_init.json.
    python tools/innerfit_init_timing.py [--reps 2] [--out profiles/innerfit_init.json]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRETCH, STRETCHES, WARMUP, FIT_REPEATS = 50, 10, 30, 5
LAUNCHES = {"camera_eval": 1, "full_eval": 5, "camera_round": 2}
UNITS = {"camera_eval": "us per evaluation", "full_eval": "us per evaluation", "camera_round": "us per round (evaluation + advance)",
         "fit_init": "ms per fitting() call", "fit_both": "ms per fitting() call", "fit_stages": "ms per fitting() call"}


def child(mode, n):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import fdcap_amd  # noqa: F401
    from fdcap_amd import capi, synth
    from fdcap_amd.innerfit import DEFAULT_INIT, DEFAULT_INTRINSICS, DEFAULT_LBFGS, InnerFitOP, init_struct
    bm, vp = synth.make_body_model(seed=0), synth.make_vposer(seed=1)
    rng = np.random.Generator(np.random.PCG64(5))
    clip = synth.make_clip(n, seed=2, num_outliers=0)
    rows = clip.body_params.astype(np.float32).copy()
    rows[:, 72:75] = np.array([0.1, -0.2, 3.0], np.float32)
    fx, fy, cx, cy = DEFAULT_INTRINSICS
    # keypoints: the rows' own joints (fdcap_opt_forward_world under the inner fit's set-up) projected, 2 px of noise
    op = InnerFitOP(bm, vp, n, iters_per_stage=0)
    op.fitting(rows, np.zeros((n, 23, 3), np.float32))
    lib, h, st = op.ctx.lib, op.ctx.handle, capi.current_stream()
    jw = torch.empty(n, 23, 3, device="cuda")
    capi.check(lib.fdcap_opt_forward_world(h, None, capi.dptr(jw), st), "fdcap_opt_forward_world")
    J = jw.cpu().numpy()
    uv = np.stack([fx * J[..., 0] / J[..., 2] + cx, fy * J[..., 1] / J[..., 2] + cy], -1)
    kp = np.concatenate([uv + 2.0 * rng.standard_normal(uv.shape), rng.uniform(0.3, 1.0, (n, 23, 1))], -1).astype(np.float32)
    out = {"mode": mode, "frames": n}
    if mode in ("fit_init", "fit_both", "fit_stages"):
        op.close()
        first = InnerFitOP(bm, vp, n, optimizer="lbfgs", init={}, orientations="both" if mode == "fit_both" else "auto")
        first.fitting(None, kp)
        cam_rows = first.camera_rows.clone()
        run = first if mode != "fit_stages" else InnerFitOP(bm, vp, n, optimizer="lbfgs")
        ms = []
        for k in range(FIT_REPEATS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run.fitting(None, kp) if mode != "fit_stages" else run.fitting(cam_rows, kp)
            torch.cuda.synchronize()
            if k:
                ms.append((time.perf_counter() - t0) * 1e3)
        out.update(values=ms, twins=int(first.tried_both.sum()), camera_rounds=first.camera_rounds, stage_rounds=run.rounds)
        print("RESULT " + json.dumps(out))
        return
    op.fitting(rows, kp)
    sg = capi.Fit2dStage(fx, fy, cx, cy, 100.0, 1.0, 4.78, 5.0, 4.78)
    ci = init_struct(dict(DEFAULT_INIT), None, DEFAULT_INTRINSICS)
    us = []
    if mode == "camera_round":
        q = dict(DEFAULT_LBFGS, max_iter=1000, max_steps=1000)
        cf = capi.LbfgsConfig(capi.XDIM, q["history"], q["max_iter"], q["max_eval"], q["max_steps"], q["max_ls"], q["lr"], q["tolerance_grad"],
                              q["tolerance_change"], q["ftol"], q["gtol"])
        turned = rows.copy()
        turned[:, 3:6] += 0.2 * rng.standard_normal((n, 3)).astype(np.float32)
        op.fitting(turned, kp)
        capi.check(lib.fdcap_opt_fit2d_guess(h, ctypes.byref(sg), ctypes.byref(ci), None, None, None, st), "fdcap_opt_fit2d_guess")
        x0, rounds_seen = op._rows_x.clone(), []
        for k in range(STRETCHES + 2):
            op._rows_x.copy_(x0)
            rounds = ctypes.c_int32(0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            capi.check(lib.fdcap_opt_fit2d_camera_lbfgs(h, ctypes.byref(sg), ctypes.byref(ci), ctypes.byref(cf), 40, ctypes.byref(rounds), st), "camera_lbfgs")
            e1.record()
            e1.synchronize()
            if k >= 2:
                us.append(e0.elapsed_time(e1) * 1e3 / max(1, rounds.value))
                rounds_seen.append(rounds.value)
        out["rounds"] = rounds_seen
    else:
        def stretch(k):
            for _ in range(k):
                if mode == "camera_eval":
                    capi.check(lib.fdcap_opt_backward_fit2d_camera(h, ctypes.byref(sg), ctypes.byref(ci), 0, st), "fdcap_opt_backward_fit2d_camera")
                else:
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
    out["values"] = us
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "innerfit_init.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.frames)
    plan = [(m, n) for n in (64, 1024) for m in ("camera_eval", "full_eval", "camera_round")] + [("fit_init", 64), ("fit_both", 64), ("fit_stages", 64)]
    runs = {}
    for rep in range(a.reps):
        for mode, n in plan:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--frames", str(n)], capture_output=True, text=True, timeout=300)
            if p.returncode != 0:                            # nothing more is started after a failure
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{mode} at {n} frames ended with status {p.returncode}")
            r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            runs.setdefault((mode, n), []).append(r)
            print(f"{n:5d} frames {mode:12s} run {rep}: median {statistics.median(r['values']):9.2f} {UNITS[mode]}", flush=True)
    table = []
    for (mode, n), rs in sorted(runs.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        med = [statistics.median(r["values"]) for r in rs]
        row = {"mode": mode, "frames": n, "unit": UNITS[mode], "launches": LAUNCHES.get(mode), "median_of_runs": statistics.median(med), "run_medians": med,
               "min": min(min(r["values"]) for r in rs), "max": max(max(r["values"]) for r in rs)}
        row.update({k: rs[0][k] for k in ("rounds", "twins", "camera_rounds", "stage_rounds") if k in rs[0]})
        table.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/innerfit_init_timing.py", "body_vertices": 10475, "layout": "23 joints", "stretch": STRETCH, "stretches_per_run": STRETCHES,
                   "runs_per_case": a.reps, "fit_repeats": FIT_REPEATS, "table": table}, f, indent=1)
        f.write("\n")
    for t in table:
        print(f"{t['frames']:5d} frames {t['mode']:12s}: {t['median_of_runs']:9.2f} {t['unit']} (runs {', '.join(f'{m:.2f}' for m in t['run_medians'])}; {t['min']:.2f} .. {t['max']:.2f})")


if __name__ == "__main__":
    main()
