#!/usr/bin/env python3
"""What the clip-level reprojection term (fdcap_opt_set_reproj) costs per iteration -> profiles/reproj_timing.json.

    python tools/reproj_timing.py [--frames 300 1024] [--iters 500] [--repeats 5] [--no-trace] [--out profiles/reproj_timing.json]

Config 3's body (bench.py build_problem: 10 475 vertices, 2 x 250 contact vertices, a 500k-point scene) at N = 300 and N = 1024, the
clip's rows carrying a camera translation of (0.1, -0.2, 3.5) (synth's clips have none; at z ~ 0 the projection is degenerate) and
random finite keypoints.  On the same tree, per N:

  * host clock: synchronised fits of `iters` iterations of ONE phase each (fdcap_opt_run with first_phase2_iter beyond the fit: all
    phase 1; 0: all phase 2), term off and on ALTERNATED, `repeats` each -> medians with their ranges, microseconds per iteration,
    and the difference on - off;
  * live launch timing (fdcap_opt_launch_timing): microseconds of every stage per phase, term off and on -- with the term off a
    phase-1 iteration runs the two pose kernels on the 12 joints the legs reach (jn = 12), with it on 23 (jn = 23): those two rows
    say where the difference goes -- next to the 6.5-9 us per-launch floor the README reports;
  * one `rocprofv3 --kernel-trace --stats` run of its own per setting (a child process of this tool: a short fit at N = 300): kernel
    launches per iteration with the term off and on, and how often pose_bwd_reproj_kernel / pose_bwd_kernel ran.

Every GPU step of the trace part runs under its own time limit; a step that fails ends the tool."""
import argparse
import ctypes
import glob
import json
import os
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WEIGHT, RHO = 2e-3, 100.0
FLOOR_US = (6.5, 9.0)                      # per-launch floor (README)
BIG = 10 ** 6


def problem(frames, iters):
    import numpy as np
    import torch
    import bench
    from fdcap_amd import innerfit
    fop, body, *_ = bench.build_problem(frames, 500_000, False, 10475, 4, 250, iters, None)
    body = body.clone()
    rng = np.random.Generator(np.random.PCG64(7))
    body[:, 72:75] = torch.tensor(np.array([0.1, -0.2, 3.5], np.float32) + 0.05 * rng.standard_normal((frames, 3)).astype(np.float32)).cuda()
    fx, fy, cx, cy = innerfit.DEFAULT_INTRINSICS
    kp = np.stack([cx + 150 * rng.standard_normal((frames, 23)), cy + 200 * rng.standard_normal((frames, 23)), rng.uniform(0.3, 1.0, (frames, 23))],
                  axis=-1).astype(np.float32)
    return fop, body, kp


def prepare(fop, body, kp, on):
    """fitting()'s prefix: rows -> 6D, init(), the term's inputs (every fdcap_opt_create switches the term off)"""
    import torch
    from fdcap_amd import capi, innerfit
    x78 = torch.empty(body.shape[0], capi.XDIM, device=body.device)
    capi.check(fop.ctx.lib.fdcap_params_75_to_78(capi.dptr(body), body.shape[0], capi.dptr(x78), capi.current_stream()), "fdcap_params_75_to_78")
    fop._mode = "global"
    fop.init(x78)
    fop.weight_reproj = WEIGHT if on else 0
    if on:
        fop._set_reproj(kp, innerfit.DEFAULT_INTRINSICS, RHO)
    torch.cuda.synchronize()


def one_phase_fit(fop, body, kp, on, phase2, iters):
    """-> host seconds of `iters` iterations of one phase, synchronised on both sides"""
    import torch
    prepare(fop, body, kp, on)
    t0 = time.perf_counter()
    fop._opt_run(0, iters, 0 if phase2 else BIG, 0, None)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def live_stages(fop, body, kp, on, iters):
    import bench
    from fdcap_amd import capi
    from fdcap_amd.fitting import first_phase2_iter
    lib, h = fop.ctx.lib, fop.ctx.handle
    n = len(bench.LT_STAGES)
    prepare(fop, body, kp, on)
    capi.check(lib.fdcap_opt_launch_timing(h, 10 * iters + 16), "fdcap_opt_launch_timing")
    fop._opt_run(0, iters, first_phase2_iter(iters), 0, None)
    us, cnt = (ctypes.c_float * (2 * n))(), (ctypes.c_int32 * (2 * n))()
    capi.check(lib.fdcap_opt_launch_timing_read(h, us, cnt), "fdcap_opt_launch_timing_read")
    capi.check(lib.fdcap_opt_launch_timing(h, 0), "fdcap_opt_launch_timing")
    out = {}
    for ph in (0, 1):
        d = {bench.LT_STAGES[i]: round(float(us[ph * n + i]), 3) for i in range(n) if cnt[ph * n + i]}
        d["sum"] = round(sum(d.values()), 3)
        out["phase1" if ph == 0 else "phase2"] = d
    return out


def med(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def measure(frames, iters, repeats):
    fop, body, kp = problem(frames, iters)
    try:
        for on in (False, True):                            # warm-up: first launches, allocations, the seeding launch
            one_phase_fit(fop, body, kp, on, False, iters)
        host = {}
        for phase2 in (False, True):
            t = {False: [], True: []}
            for _ in range(repeats):
                for on in (False, True):                    # alternated
                    t[on].append(one_phase_fit(fop, body, kp, on, phase2, iters) * 1e6 / iters)
            off, on_ = med(t[False]), med(t[True])
            host["phase2" if phase2 else "phase1"] = {"off_us_per_iter": off, "on_us_per_iter": on_, "on_minus_off_us": on_["median"] - off["median"]}
        live = {"off": live_stages(fop, body, kp, False, iters), "on": live_stages(fop, body, kp, True, iters)}
        p1 = {k: {"jn12_term_off_us": live["off"]["phase1"].get(k), "jn23_term_on_us": live["on"]["phase1"].get(k)} for k in ("pose_fwd", "pose_bwd")}
    finally:
        fop.close()
    return {"frames": frames, "iters": iters, "repeats": repeats, "host_clock": host, "live_launch_timing_us": live,
            "phase1_pose_kernels": p1, "per_launch_floor_us": list(FLOOR_US)}


def child_fit(on, frames, iters):
    """the traced program: one plain fit, nothing else"""
    import torch
    fop, body, kp = problem(frames, iters)
    prepare(fop, body, kp, on)
    from fdcap_amd.fitting import first_phase2_iter
    fop._opt_run(0, iters, first_phase2_iter(iters), 0, None)
    torch.cuda.synchronize()
    fop.close()
    print("RESULT ok")


def trace(frames=300, iters=50):
    """rocprofv3 --kernel-trace --stats around a child of its own, term off then on -> kernel launches per setting"""
    out = {"frames": frames, "iters": iters}
    for on in (False, True):
        d = tempfile.mkdtemp(prefix="reproj_trace_")
        cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "r", "--", sys.executable,
               os.path.abspath(__file__), "--child", "on" if on else "off", "--frames", str(frames), "--iters", str(iters)]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if p.returncode != 0 or "RESULT ok" not in p.stdout:
            raise SystemExit(f"traced child failed ({p.returncode}): {p.stderr[-1500:]}")
        calls = {}
        for db in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
            for name, n in sqlite3.connect(db).execute("select name, total_calls from top_kernels"):
                short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                calls[short] = calls.get(short, 0) + int(n)
        if not calls:
            raise SystemExit(f"no kernel statistics under {d}: {os.listdir(d)}")
        out["on" if on else "off"] = {"kernel_launches": sum(calls.values()),
                                      "pose_bwd_kernel": sum(v for k, v in calls.items() if k.endswith("pose_bwd_kernel")),
                                      "pose_bwd_reproj_kernel": sum(v for k, v in calls.items() if k.endswith("pose_bwd_reproj_kernel"))}
    out["launches_per_iteration_on_minus_off"] = (out["on"]["kernel_launches"] - out["off"]["kernel_launches"]) / iters
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, nargs="+", default=[300, 1024])
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproj_timing.json"))
    ap.add_argument("--child", choices=("off", "on"), default=None, help="(internal) the traced program")
    a = ap.parse_args()
    if a.child:
        return child_fit(a.child == "on", a.frames[0], a.iters)
    res = {"tool": "tools/reproj_timing.py", "weight_reproj": WEIGHT, "rho": RHO, "sizes": [measure(f, a.iters, a.repeats) for f in a.frames]}
    if not a.no_trace:
        res["kernel_trace"] = trace()
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    for s in res["sizes"]:
        for ph, v in s["host_clock"].items():
            print(f"N={s['frames']} {ph}: off {v['off_us_per_iter']['median']:.2f} us/iter, on {v['on_us_per_iter']['median']:.2f}, on - off {v['on_minus_off_us']:+.2f}")
        print(f"N={s['frames']} phase-1 pose kernels: {s['phase1_pose_kernels']}")
    if "kernel_trace" in res:
        print("kernel trace:", res["kernel_trace"])


if __name__ == "__main__":
    main()
