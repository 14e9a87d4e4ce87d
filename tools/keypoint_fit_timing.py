#!/usr/bin/env python3
"""Cost of one objective evaluation of the inner fit (forward, loss, backward) on the 23-joint layout and on mapped keypoints,
V = 10 475 synthetic body, 64 and 1024 frames:
  (a) the 23-joint path of another build of the library (--parent-lib: the commit before the keypoint map),
  (b) the 23-joint path of this tree,
  (c) 67 mapped keypoints (BODY_25 + both hands: 21 vertices, 30 finger joints),
  (d) 67 + 51 face landmarks (barycentric triples: 153 more vertices when no two landmarks share one),
(c) and (d) with the set's blend products inside the kernel (ck, dk: five launches, as (a) and (b)) and as panel products around it
(cp, dp: seven launches) -- FDCAP_KP_BLEND pinned either way.
Device events around stretches of fdcap_opt_backward_fit2d calls; every case runs in a process of its own, the cases alternated
(a, b, ck, cp, dk, dp, a, b, ..) so that drift of the machine falls on all alike.  Writes profiles/keypoints_fit.json.
    python tools/keypoint_fit_timing.py [--parent-lib PATH] [--reps 3] [--out profiles/keypoints_fit.json]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fdcap_set_keypoint_map", "fdcap_opt_set_keypoints_mapped", "fdcap_debug_keypoints3d")
STRETCH, STRETCHES, WARMUP = 50, 12, 30


def child(case, n):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import fdcap_amd  # noqa: F401
    from fdcap_amd import capi, synth
    from fdcap_amd.innerfit import DEFAULT_INTRINSICS, OPENPOSE_BODY25, OPENPOSE_LHAND, OPENPOSE_RHAND, InnerFitOP, KeypointMap
    if case == "a":                                          # a build without the map: bind what it exports
        for s in NEW_SYMBOLS:
            capi.SYMBOLS.pop(s, None)
    bm, vp = synth.make_body_model(seed=0), synth.make_vposer(seed=1)
    V = bm.v_template.shape[0]
    rng = np.random.Generator(np.random.PCG64(5))
    kmap = None
    if case[0] in "cd":
        idx = list(OPENPOSE_BODY25 + OPENPOSE_LHAND + OPENPOSE_RHAND) + (list(range(76, 127)) if case[0] == "d" else [])
        ids = rng.permutation(V)
        kmap = KeypointMap.from_smplx_indices(idx, ids[:21], ids[21:21 + 153].reshape(51, 3), rng.dirichlet((1.0, 1.0, 1.0), 51))
    nkp = 23 if kmap is None else len(kmap)
    clip = synth.make_clip(n, seed=2, num_outliers=0)
    rows = clip.body_params.astype(np.float32).copy()
    rows[:, 72:75] = np.array([0.1, -0.2, 3.5], np.float32)
    kp = np.concatenate([rng.uniform(100, 1100, (n, nkp, 2)), rng.uniform(0.3, 1.0, (n, nkp, 1))], -1).astype(np.float32)
    op = InnerFitOP(bm, vp, n, iters_per_stage=0, keypoint_map=kmap)
    op.fitting(rows, kp)
    lib, h = op.ctx.lib, op.ctx.handle
    sg = capi.Fit2dStage(*DEFAULT_INTRINSICS, 100.0, 1.0, 4.78, 5.0, 4.78)
    st = capi.current_stream()

    def stretch(k):
        for _ in range(k):
            capi.check(lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 0, st), "fdcap_opt_backward_fit2d")
    stretch(WARMUP)
    torch.cuda.synchronize()
    us = []
    for _ in range(STRETCHES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        stretch(STRETCH)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / STRETCH)
    op.close()
    print("RESULT " + json.dumps({"case": case, "frames": n, "keypoints": nkp, "set_vertices": 0 if kmap is None else int(len(set(
        kmap.tri[kmap.joint < 0].reshape(-1).tolist())) + len(set(kmap.joint[kmap.joint >= 23].tolist()))), "us_per_eval": us}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoints_fit.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.frames)
    import statistics
    cases = (["a"] if a.parent_lib else []) + ["b", "ck", "cp", "dk", "dp"]
    runs = {}
    for n in (64, 1024):
        for rep in range(a.reps):
            for case in cases:
                env = dict(os.environ)
                env.pop("FDCAP_KP_BLEND", None)
                if case == "a":
                    env["FDCAP_LIB"] = os.path.abspath(a.parent_lib)
                if len(case) == 2:
                    env["FDCAP_KP_BLEND"] = "kernel" if case[1] == "k" else "panel"
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--frames", str(n)], env=env, capture_output=True,
                                   text=True, timeout=300)
                if p.returncode != 0:                        # nothing more is started after a failure
                    sys.stderr.write(p.stdout + p.stderr)
                    raise SystemExit(f"case {case} at {n} frames ended with status {p.returncode}")
                r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
                runs.setdefault((case, n), []).append(r)
                print(f"{n:5d} frames ({case:2s}) run {rep}: median {statistics.median(r['us_per_eval']):8.2f} us per evaluation", flush=True)
    table = []
    for (case, n), rs in sorted(runs.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        med = [statistics.median(r["us_per_eval"]) for r in rs]
        table.append({"case": case, "frames": n, "keypoints": rs[0]["keypoints"], "set_vertices": rs[0]["set_vertices"], "launches_per_eval": 7 if case.endswith("p") else 5,
                      "us_per_eval_median_of_runs": statistics.median(med), "us_per_eval_run_medians": med,
                      "us_per_eval_min": min(min(r["us_per_eval"]) for r in rs), "us_per_eval_max": max(max(r["us_per_eval"]) for r in rs)})
    out = {"tool": "tools/keypoint_fit_timing.py", "body_vertices": 10475, "stretch": STRETCH, "stretches_per_run": STRETCHES, "runs_per_case": a.reps,
           "cases": {"a": "23 joints, the build given as --parent-lib", "b": "23 joints, this tree", "ck": "67 mapped keypoints (BODY_25 + hands), blend products in the kernel",
                     "cp": "the same, panel products around the kernel", "dk": "67 + 51 face landmarks, blend products in the kernel",
                     "dp": "the same, panel products around the kernel"}, "table": table}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for t in table:
        print(f"{t['frames']:5d} frames ({t['case']:2s}) {t['keypoints']:3d} keypoints: {t['us_per_eval_median_of_runs']:8.2f} us per evaluation "
              f"(runs {', '.join(f'{m:.2f}' for m in t['us_per_eval_run_medians'])}; stretches {t['us_per_eval_min']:.2f} .. {t['us_per_eval_max']:.2f})")


if __name__ == "__main__":
    main()
