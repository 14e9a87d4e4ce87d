#!/usr/bin/env python3
"""Cost of the body-model operator with the fitted face: fdcap_smplx_forward_face / fdcap_smplx_backward_face with jaw_pose and expression
both given, next to fdcap_smplx_forward / fdcap_smplx_backward of this tree and of another build of the library (--parent-lib: the commit
before), on the V = 10 475 synthetic body at B = 64 and B = 1024:
  parent   the build given as --parent-lib, the entry points without `_face`
  plain    this tree, the entry points without `_face`
  face     this tree, the `_face` entry points, both arrays given
  jaw      ... jaw_pose alone          psi   ... expression alone
forward (vertices and joints) and backward (gradients on vertices and joints, all eight input gradients asked for) timed apart.
Device events around stretches of 50 calls; every case runs in a process of its own, the cases alternated so that drift of the machine
falls on all alike.  Nothing more is started after a case that fails.  Next to every difference the table gives its BYTE FLOOR: the bytes
the route adds, counted from shapes, over 6.3 TB/s --
  forward   expr_offsets_kernel reads and writes the offsets in place (2 x 12 B V), face_fwd_kernel reads A and PF and writes A' and PF',
            blend_forward reads PF' where it read PF (no change);
  backward  the same, plus expr_dpsi_kernel's read of d offsets (12 B V) and face_bwd_kernel's A, d A' in and d A out.
And the inner fit's evaluation with the self-interpenetration term (fdcap_opt_backward_fit2d on synth.make_body_mesh(10475), 64 frames,
67 mapped keypoints, the blend products in the kernel): `fit_parent` / `fit_off` the term on with the face fixed, parent build against this
tree; `fit_on` the same with fdcap_opt_set_fit2d_collision_face and the jaw and psi free.
Writes profiles/face_mesh.json.
    python tools/face_mesh_timing.py --parent-lib PATH [--reps 2] [--out profiles/face_mesh.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fdcap_body_forward_face", "fdcap_world_mesh_face", "fdcap_smplx_forward_face", "fdcap_smplx_backward_face",
               "fdcap_opt_set_fit2d_collision_face")
STRETCH, STRETCHES, WARMUP = 50, 10, 10
FIT_STRETCH = 10                                             # evaluations per stretch of the inner fit's cases (milliseconds each)
HBM_BYTES_PER_US = 6.3e6                                     # 6.3 TB/s
MODES = ("parent", "plain", "face", "jaw", "psi", "fit_parent", "fit_off", "fit_on")


def extra_bytes(mode, what, B, V):
    """bytes the route moves on top of the plain entry point, from shapes alone"""
    if mode in ("parent", "plain") or mode.startswith("fit_"):
        return 0
    jaw, psi = mode in ("face", "jaw"), mode in ("face", "psi")
    a, pf, off = B * 55 * 12 * 4, B * 496 * 4, B * 3 * V * 4
    n = 2 * a + (2 * pf if jaw else 0) + (2 * off if psi else 0)           # face_fwd_kernel, expr_offsets_kernel
    if what == "backward":
        n += 3 * a + (off if psi else 0)                                  # face_bwd_kernel, expr_dpsi_kernel
    return n


def child_fit(mode, n):
    """one evaluation of the inner fit with the term: fit_parent / fit_off (the face fixed), fit_on (jaw and psi free, the term follows)"""
    import ctypes
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import fdcap_amd  # noqa: F401
    from fdcap_amd import capi, synth
    from fdcap_amd.innerfit import DEFAULT_INTRINSICS, OPENPOSE_BODY25, OPENPOSE_LHAND, OPENPOSE_RHAND, InnerFitOP, KeypointMap
    if mode == "fit_parent":
        for s in NEW_SYMBOLS:
            capi.SYMBOLS.pop(s, None)
    bm, part, parent = synth.make_body_mesh(seed=0)
    vp = synth.make_vposer(seed=1)
    V = bm.v_template.shape[0]
    rng = np.random.Generator(np.random.PCG64(5))
    ids = rng.permutation(V)
    kmap = KeypointMap.from_smplx_indices(list(OPENPOSE_BODY25 + OPENPOSE_LHAND + OPENPOSE_RHAND), ids[:21])
    nkp = len(kmap)
    rows = synth.make_clip(n, seed=2, num_outliers=0).body_params.astype(np.float32).copy()
    rows[:, 72:75] = np.array([0.1, -0.2, 3.5], np.float32)
    kp = np.concatenate([rng.uniform(100, 1100, (n, nkp, 2)), rng.uniform(0.3, 1.0, (n, nkp, 1))], -1).astype(np.float32)
    on = mode == "fit_on"
    coll = dict(face_part=part, part_parent=parent, weights=(1.0,) * 5)
    if on:
        coll["follow_face"] = True
    op = InnerFitOP(bm, vp, n, iters_per_stage=0, keypoint_map=kmap, collision=coll, fit_jaw=on, fit_expression=on)
    op.fitting(rows, kp)
    lib, h, st = op.ctx.lib, op.ctx.handle, capi.current_stream()
    if on:
        jaw = torch.tensor(0.1 * rng.standard_normal((n, 3)).astype(np.float32), device="cuda")
        psi = torch.tensor(0.5 * rng.standard_normal((n, 10)).astype(np.float32), device="cuda")
        capi.check(lib.fdcap_opt_set_jaw(h, capi.dptr(jaw), st), "fdcap_opt_set_jaw")
        capi.check(lib.fdcap_opt_set_expression(h, capi.dptr(psi), st), "fdcap_opt_set_expression")
    sg = capi.Fit2dStage(*DEFAULT_INTRINSICS, 100.0, 1.0, 4.78, 5.0, 4.78)
    us = []
    for k in range(STRETCHES + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(FIT_STRETCH):
            capi.check(lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 0, st), "fdcap_opt_backward_fit2d")
        e1.record()
        e1.synchronize()
        if k:
            us.append(e0.elapsed_time(e1) * 1e3 / FIT_STRETCH)
    op.close()
    print("RESULT " + json.dumps({"mode": mode, "what": "evaluation", "B": n, "V": V, "us": us}))


def child(mode, what, B):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import fdcap_amd  # noqa: F401
    from fdcap_amd import capi, synth
    if mode.startswith("fit_"):
        return child_fit(mode, B)
    if mode == "parent":                                     # a build without the new entry points: bind what it exports
        for s in NEW_SYMBOLS:
            capi.SYMBOLS.pop(s, None)
    bm, vp = synth.make_body_model(seed=0), synth.make_vposer(seed=1)
    V = bm.v_template.shape[0]
    ctx = capi.Context(bm, vp)
    lib, h, st = ctx.lib, ctx.handle, capi.current_stream()
    rng = np.random.Generator(np.random.PCG64(5))
    dev = lambda *s, k=1.0: torch.tensor((k * rng.standard_normal(s)).astype(np.float32), device="cuda")
    ins = [dev(B, 3, k=0.8), dev(B, 63, k=0.4), dev(B, 10, k=0.5), dev(B, 12, k=0.3), dev(B, 12, k=0.3), dev(B, 3)]
    jaw = dev(B, 3, k=0.2) if mode in ("face", "jaw") else None
    psi = dev(B, 10, k=1.5) if mode in ("face", "psi") else None
    verts, joints = torch.empty(B, V, 3, device="cuda"), torch.empty(B, 55, 3, device="cuda")
    gv, gj = dev(B, V, 3), dev(B, 55, 3)
    gs = [torch.empty_like(t) for t in ins]
    gjaw = None if jaw is None else torch.empty_like(jaw)
    gpsi = None if psi is None else torch.empty_like(psi)
    p, g = [capi.dptr(t) for t in ins], [capi.dptr(t) for t in gs]
    face = mode in ("face", "jaw", "psi")

    def call():
        if what == "forward" and face:
            e = lib.fdcap_smplx_forward_face(h, *p, B, capi.dptr(jaw), capi.dptr(psi), capi.dptr(verts), capi.dptr(joints), st)
        elif what == "forward":
            e = lib.fdcap_smplx_forward(h, *p, B, capi.dptr(verts), capi.dptr(joints), st)
        elif face:
            e = lib.fdcap_smplx_backward_face(h, *p, B, capi.dptr(jaw), capi.dptr(psi), capi.dptr(gv), capi.dptr(gj), *g, capi.dptr(gjaw),
                                              capi.dptr(gpsi), st)
        else:
            e = lib.fdcap_smplx_backward(h, *p, B, capi.dptr(gv), capi.dptr(gj), *g, st)
        capi.check(e, f"{what} ({mode})")
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(STRETCHES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STRETCH):
            call()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / STRETCH)
    ctx.close()
    print("RESULT " + json.dumps({"mode": mode, "what": what, "B": B, "V": V, "us": us}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--parent-lib", required=False)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--fit-only", action="store_true", help="the inner fit's three cases alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_mesh.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.batch)
    modes = [m for m in MODES[:5] if m != "parent" or a.parent_lib]
    plan = [] if a.fit_only else [(m, what, B) for B in (64, 1024) for what in ("forward", "backward") for m in modes]
    plan += [(m, "evaluation", 64) for m in MODES[5:] if m != "fit_parent" or a.parent_lib]
    runs = {}
    for rep in range(a.reps):
        for mode, what, B in plan:
            env = dict(os.environ)
            if mode in ("parent", "fit_parent"):
                env["FDCAP_LIB"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, what, "--batch", str(B)], env=env, capture_output=True,
                               text=True, timeout=600)
            if p.returncode != 0:                            # nothing more is started after a failure
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{mode} {what} at B = {B} ended with status {p.returncode}")
            r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            runs.setdefault((mode, what, B), []).append(r)
            print(f"B {B:5d} {what:8s} {mode:7s} run {rep}: median {statistics.median(r['us']):9.2f} us", flush=True)
    table = []
    for (mode, what, B), rs in sorted(runs.items(), key=lambda kv: (kv[0][2], kv[0][1], MODES.index(kv[0][0]))):
        med = [statistics.median(r["us"]) for r in rs]
        nb = extra_bytes(mode, what, B, rs[0]["V"])
        table.append({"mode": mode, "what": what, "B": B, "unit": "us per call", "median_of_runs": statistics.median(med), "run_medians": med,
                      "min": min(min(r["us"]) for r in rs), "max": max(max(r["us"]) for r in rs), "extra_bytes": nb,
                      "byte_floor_us": nb / HBM_BYTES_PER_US})
    base = {(t["what"], t["B"]): t["median_of_runs"] for t in table if t["mode"] in (("parent", "fit_parent") if a.parent_lib else ("plain", "fit_off"))}
    for t in table:
        t["over_baseline_us"] = t["median_of_runs"] - base[(t["what"], t["B"])]
    out = {"tool": "tools/face_mesh_timing.py", "body_vertices": 10475, "stretch": STRETCH, "stretches_per_run": STRETCHES, "runs_per_case": a.reps,
           "baseline": "parent" if a.parent_lib else "plain", "table": table}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for t in table:
        print(f"B {t['B']:5d} {t['what']:8s} {t['mode']:7s}: {t['median_of_runs']:9.2f} us (runs {', '.join(f'{m:.2f}' for m in t['run_medians'])}; "
              f"stretches {t['min']:.2f} .. {t['max']:.2f}); over the baseline {t['over_baseline_us']:+8.2f} us, byte floor {t['byte_floor_us']:.2f} us")


if __name__ == "__main__":
    main()
