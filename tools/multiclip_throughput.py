#!/usr/bin/env python3
"""Throughput of a batch of clips (fitting.ClipBatchFitter, fdcap_opt_create_clips) on BASELINE config 3's body and scene
(V = 10 475, 500 contact vertices, 500 k scene points) at the reference's clip length N = 300, 500 iterations:
  - K in {1, 2, 3, 4, 6, 8} clips per batch: ms per batch (host clock around fits that end in a synchronise, after one warm-up
    fit of that K), frames/s and clips/s;
  - 12 clips through the batch driver (one context for all; default K) against 12 FittingOP fits in one process (a context
    each), host clock from the first constructor to the last result on the host;
  - the live per-launch table at K = 3 (fdcap_opt_launch_timing, as tools/launch_times.py reads it).
Prints one JSON line (profiles/r7_multiclip300.json).
--lengths n0,n1,... (may be repeated): instead of the sweep, a batch of clips of THOSE lengths (fdcap_opt_create_clips_var when they
differ) under the same protocol -- one warm-up fit, R timed fits that end in a synchronise -- with ms per batch, us per iteration,
frames/s and the live per-launch table; one entry per --lengths, all on one fitter.
--mode local: instead of the sweep, mode 'local' (first loop + detect_contact + the 0.4 x 500 iterations of the second loop over
all 10 475 vertices): K = 1 and K = 3 clips of 300 frames through ClipBatchFitter.fit(mode='local') against K sequential stand-alone
FittingOP mode-'local' fits in the same process (their contexts built before the clock starts) -- one warm-up each, then R rounds
that alternate the two, each timed by the host clock around fits that end with the results on the host; medians, clips/s and the
ratio (profiles/multiclip300_local.json).
--mode dct: instead of the sweep, mode 'dct' at its 10 000 iterations (9 500 first-phase iterations in one launch, a no-op, 499 of the
second phase): K = 1, 3 and 8 clips of 300 frames through ClipBatchFitter.fit(mode='dct') against K sequential stand-alone FittingOP
mode-'dct' fits in the same process, under mode 'local''s protocol (one warm-up each, R rounds that alternate the two, medians), and
the batch's two phases on their own -- fdcap_opt_run_dct cut at the phase switch, each stretch between two device events
(profiles/multiclip300_dct.json).
--scenes: instead of the sweep, K = 3 clips of 300 frames on three different 500 k-point scenes: the multi-scene batch through the
one-launch segmented search, the same batch searched segment after segment (FDCAP_NN_SEGMENTS=loop), and three one-clip fits that
each register their scene first -- alternated in one process, medians of R, and the live per-launch tables of the two batches
(profiles/multiscene300.json).  --scenes-c-only: the third alone, through the one-scene interface (any tree).
usage: python tools/multiclip_throughput.py [--reps R] [--out FILE] [--mode local|dct] [--lengths n0,n1,...]... [--scenes]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

N, ITERS, NS, KS = 300, 500, 500_000, (1, 2, 3, 4, 6, 8)


def main():
    argv = sys.argv[1:]
    reps, out, lengths, mode, multi_scene = 3, None, [], "global", None
    while argv:
        if argv[0] in ("--scenes", "--scenes-c-only"):
            multi_scene, argv = argv[0], argv[1:]
            continue
        if argv[0] == "--mode" and len(argv) > 1 and argv[1] in ("global", "local", "dct"):
            mode, argv = argv[1], argv[2:]
        elif argv[0] == "--reps":
            reps, argv = int(argv[1]), argv[2:]
        elif argv[0] == "--out":
            out, argv = argv[1], argv[2:]
        elif argv[0] == "--lengths":
            lengths.append([int(t) for t in argv[1].split(",")])
            argv = argv[2:]
        else:
            raise SystemExit(__doc__)
    import fdcap_amd  # noqa: F401
    from fdcap_amd import cli, synth
    from fdcap_amd.fitting import ClipBatchFitter, FittingOP
    from fdcap_amd.io import read_camerapose
    bm = synth.make_body_model(10475, seed=0)
    vp = synth.make_vposer(seed=1)
    scene = synth.make_scene(NS, seed=2)
    left, right = synth.make_contact_ids(bm.v_template, per_part=250, seed=4)
    vid = np.concatenate([left, right])
    if multi_scene:
        if lengths or mode != "global":
            raise SystemExit("--scenes measures three 300-frame clips in mode 'global': not with --lengths / --mode")
        return scenes_mode(reps, out, bm, vp, vid, multi_scene == "--scenes-c-only")
    if mode in ("local", "dct"):
        if lengths:
            raise SystemExit(f"--mode {mode} measures clips of 300 frames: not with --lengths")
        return (local_mode if mode == "local" else dct_mode)(reps, out, bm, vp, scene, vid)
    if lengths:
        return ragged(lengths, reps, out, bm, vp, scene, vid)
    clips = []
    for k in range(12):
        c = synth.make_clip(N, seed=100 + k)
        clips.append((c.body_params, read_camerapose(c.camerapose_lines)))
    res = {"problem": {"verts": 10475, "contacts": len(vid), "scene": NS, "frames_per_clip": N, "iters": ITERS}, "sweep": []}

    fitter = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    fitter.set_scene(scene)

    def fit(K):
        r = fitter.fit(clips[:K])
        return [(b.cpu(), s, c.cpu()) for b, s, c in r]

    for K in KS:
        fit(K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fit(K)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        res["sweep"].append({"K": K, "rows": K * N, "ms_per_batch": dt * 1e3, "frames_per_s": K * N / dt, "clips_per_s": K / dt})
        print(f"K {K}: {dt * 1e3:8.2f} ms per batch  {K * N / dt:9.0f} frames/s  {K / dt:7.2f} clips/s", file=sys.stderr, flush=True)
    by_k = {r["K"]: r for r in res["sweep"]}
    res["speedup_k3_over_k1_frames_per_s"] = by_k[3]["frames_per_s"] / by_k[1]["frames_per_s"]

    # the live per-launch table at K = 3 (the same fit, one event per launch boundary)
    fit(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit(3)
    torch.cuda.synchronize()
    live = bench.time_all_launches(fitter, lambda: fit(3), ITERS, time.perf_counter() - t0)
    res["launch_table_k3"] = {ph: {k: round(v.get("us_corrected", v["us"]), 2) for k, v in live[ph].items()} for ph in ("phase1", "phase2")}
    fitter.close()
    torch.cuda.empty_cache()

    # 12 clips: one persistent batch driver vs a FittingOP (context, scene, contact ids) per clip, both in this process
    k_def = cli.batch_size(N)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    f.set_scene(scene)
    for j in range(0, 12, k_def):
        [(b.cpu(), s, c.cpu()) for b, s, c in f.fit(clips[j:j + k_def])]
    f.close()
    torch.cuda.synchronize()
    t_batch = time.perf_counter() - t0
    t0 = time.perf_counter()
    for body, cam in clips:
        fop = FittingOP({"num_iter": ITERS}, {}, N, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid, camera_ext=cam)
        b, s, c = fop.fitting(torch.tensor(body).cuda(), "global")
        b.cpu(), c.cpu()
        fop.close()
    torch.cuda.synchronize()
    t_single = time.perf_counter() - t0
    res["twelve_clips"] = {"clips_per_batch": k_def, "batch_driver_s": t_batch, "fittingop_each_s": t_single,
                           "batch_driver_frames_per_s": 12 * N / t_batch, "fittingop_each_frames_per_s": 12 * N / t_single,
                           "note": "host clock from the first constructor to the last result on the host; model and scene arrays in memory"}
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "w") as fh:
            fh.write(line + "\n")


def scenes_mode(reps, out, bm, vp, vid, c_only):
    """K = 3 clips of N frames on three DIFFERENT 500 k-point scenes, mode 'global': (a) one multi-scene batch through the one-launch
    segmented search, (b) the same batch with FDCAP_NN_SEGMENTS=loop (one search launch set per segment), (c) three one-clip fits
    through one ClipBatchFitter that registers each clip's scene before its fit -- what a run of videos with a scene each cost before
    scenes could share a batch.  One warm-up each, then R rounds that alternate the three, each timed by the host clock around fits
    that end with the results on the host; medians.  (a) and (b) register their scenes once (the slots keep them by key).
    c_only: only (c), through nothing but the one-scene interface -- runs on a tree without scene slots too."""
    from fdcap_amd import synth
    from fdcap_amd.fitting import ClipBatchFitter
    from fdcap_amd.io import read_camerapose
    K = 3
    clips, scenes = [], []
    for k in range(K):
        c = synth.make_clip(N, seed=100 + k)
        clips.append((c.body_params, read_camerapose(c.camerapose_lines)))
        scenes.append(synth.make_scene(NS, seed=2 + 10 * k) + np.array([0.0, 0.0, 0.05 * k], np.float32))
    fitter = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    fitter_c = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)      # (its own context: (c) replaces slot 0's scene)

    def batch(loop):
        if loop:
            os.environ["FDCAP_NN_SEGMENTS"] = "loop"
        try:
            t0 = time.perf_counter()
            r = [(b.cpu(), s, c.cpu()) for b, s, c in fitter.fit(clips, scenes=[(f"scene{k}", scenes[k]) for k in range(K)], clip_scene=list(range(K)))]
            torch.cuda.synchronize()
            return time.perf_counter() - t0, r
        finally:
            os.environ.pop("FDCAP_NN_SEGMENTS", None)

    def each():
        t0 = time.perf_counter()
        r = []
        for k in range(K):
            (b, s, c), = fitter_c.fit([clips[k]], scenes[k], scene_key=f"one{k}")
            r.append((b.cpu(), s, c.cpu()))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    res = {"problem": {"verts": 10475, "contacts": len(vid), "scene": NS, "scenes": K, "frames_per_clip": N, "iters": ITERS, "clips": K,
                       "reps": reps}}
    ways = {"c_one_clip_fits_scene_registered_per_clip": each} if c_only else \
        {"a_segmented_launch": lambda: batch(False), "b_segment_loop": lambda: batch(True), "c_one_clip_fits_scene_registered_per_clip": each}
    first = {name: fn()[1] for name, fn in ways.items()}                       # (warm-up; and the three ways agree)
    if not c_only:
        ra, rb, rc = first["a_segmented_launch"], first["b_segment_loop"], first["c_one_clip_fits_scene_registered_per_clip"]
        res["a_equals_b_bit_for_bit"] = all(torch.equal(x[0], y[0]) and torch.equal(x[2], y[2]) for x, y in zip(ra, rb))
        res["max_abs_body_difference_a_c"] = max(float((x[0] - y[0]).abs().max()) for x, y in zip(ra, rc))
    times = {name: [] for name in ways}
    for _ in range(reps):
        for name, fn in ways.items():
            times[name].append(fn()[0])
    for name, ts in times.items():
        m = float(np.median(ts))
        res[name] = {"ms": m * 1e3, "ms_all": [t * 1e3 for t in ts], "frames_per_s": K * N / m, "clips_per_s": K / m}
        print(f"{name}: {m * 1e3:8.2f} ms  {K * N / m:9.0f} frames/s", file=sys.stderr, flush=True)
    if not c_only:
        for name, loop in (("a_segmented_launch", False), ("b_segment_loop", True)):
            live = bench.time_all_launches(fitter, lambda: batch(loop), ITERS, res[name]["ms"] * 1e-3)
            res[name]["launch_table"] = {ph: {k: round(v.get("us_corrected", v["us"]), 2) for k, v in live[ph].items()} for ph in ("phase1", "phase2")}
    fitter.close()
    fitter_c.close()
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "w") as fh:
            fh.write(line + "\n")


def ragged(lengths, reps, out, bm, vp, scene, vid):
    """One entry per list of lengths: the sweep's protocol on a batch of clips of those lengths."""
    from fdcap_amd import synth
    from fdcap_amd.fitting import ClipBatchFitter
    from fdcap_amd.io import read_camerapose
    res = {"problem": {"verts": 10475, "contacts": len(vid), "scene": NS, "iters": ITERS, "reps": reps}, "batches": []}
    fitter = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    fitter.set_scene(scene)
    for lens in lengths:
        clips = []
        for k, n in enumerate(lens):
            c = synth.make_clip(n, seed=100 + k)
            clips.append((c.body_params, read_camerapose(c.camerapose_lines)))

        def fit():
            return [(b.cpu(), s, c.cpu()) for b, s, c in fitter.fit(clips)]

        fit()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fit()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        dt = float(np.median(times))
        live = bench.time_all_launches(fitter, fit, ITERS, dt)
        rows = sum(lens)
        entry = {"lengths": lens, "rows": rows, "ms_per_batch": dt * 1e3, "ms_per_batch_all": [t * 1e3 for t in times],
                 "us_per_iter": dt * 1e6 / ITERS, "frames_per_s": rows / dt, "clips_per_s": len(lens) / dt,
                 "launch_table": {ph: {k: round(v.get("us_corrected", v["us"]), 2) for k, v in live[ph].items()} for ph in ("phase1", "phase2")}}
        res["batches"].append(entry)
        print(f"lengths {lens}: {dt * 1e3:8.2f} ms per batch  {rows / dt:9.0f} frames/s", file=sys.stderr, flush=True)
    fitter.close()
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "w") as fh:
            fh.write(line + "\n")


def local_mode(reps, out, bm, vp, scene, vid):
    """K = 1 and K = 3 clips of N frames in mode 'local': one batch against K stand-alone fits, alternating."""
    from fdcap_amd import synth
    from fdcap_amd.fitting import LOCAL_SECOND_LOOP, ClipBatchFitter, FittingOP
    from fdcap_amd.io import read_camerapose
    clips = []
    for k in range(3):
        c = synth.make_clip(N, seed=100 + k)
        clips.append((c.body_params, read_camerapose(c.camerapose_lines)))
    fitter = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    fitter.set_scene(scene)
    fops = [FittingOP({"num_iter": ITERS}, {}, N, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid, camera_ext=cam)
            for _, cam in clips]
    bodies = [torch.tensor(body).cuda() for body, _ in clips]

    def batch(K):
        t0 = time.perf_counter()
        r = [(b.cpu(), s, c.cpu()) for b, s, c in fitter.fit(clips[:K], mode="local")]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def alone(K):
        t0 = time.perf_counter()
        r = []
        for k in range(K):
            b, s, c = fops[k].fitting(bodies[k], "local")
            r.append((b.cpu(), s, c.cpu()))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    res = {"problem": {"verts": 10475, "contacts": len(vid), "scene": NS, "frames_per_clip": N, "iters": ITERS,
                       "second_loop_iters": int(LOCAL_SECOND_LOOP * ITERS), "mode": "local", "reps": reps}, "sweep": []}
    for K in (1, 3):
        _, rb = batch(K)
        _, ra = alone(K)
        # (same forms or not, the two must agree closely: the measurement compares two ways to the same result)
        worst = max(float((b[0] - a[0]).abs().max()) for b, a in zip(rb, ra))
        tb, ta = [], []
        for _ in range(reps):
            tb.append(batch(K)[0])
            ta.append(alone(K)[0])
        mb, ma = float(np.median(tb)), float(np.median(ta))
        res["sweep"].append({"K": K, "rows": K * N, "batch_ms": mb * 1e3, "batch_ms_all": [t * 1e3 for t in tb],
                             "stand_alone_ms": ma * 1e3, "stand_alone_ms_all": [t * 1e3 for t in ta],
                             "batch_clips_per_s": K / mb, "stand_alone_clips_per_s": K / ma, "batch_over_stand_alone": ma / mb,
                             "max_abs_body_difference": worst})
        print(f"K {K}: batch {mb * 1e3:8.2f} ms ({K / mb:6.2f} clips/s)  stand-alone x{K} {ma * 1e3:8.2f} ms ({K / ma:6.2f} clips/s)  "
              f"ratio {ma / mb:5.2f}", file=sys.stderr, flush=True)
    fitter.close()
    for f in fops:
        f.close()
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "w") as fh:
            fh.write(line + "\n")


def dct_mode(reps, out, bm, vp, scene, vid):
    """K = 1, 3 and 8 clips of N frames in mode 'dct': one batch against K stand-alone fits, alternating; the batch's two phases."""
    import ctypes
    from fdcap_amd import capi, synth
    from fdcap_amd.fitting import DCT_NUM_ITER, DCT_PHASE1_WEIGHT, DCT_PHASE2, ClipBatchFitter, FittingOP, dct_first_phase2_iter
    from fdcap_amd.io import load_dct_base, read_camerapose
    ks = (1, 3, 8)
    D = load_dct_base(None)
    rng = np.random.Generator(np.random.PCG64(7))
    clips, c0 = [], []
    for k in range(max(ks)):
        c = synth.make_clip(N, seed=100 + k)
        clips.append((c.body_params, read_camerapose(c.camerapose_lines)))
        c0.append(rng.standard_normal((N // 60, 23, 3, 5)).astype(np.float32))
    fitter = ClipBatchFitter({}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    fitter.set_scene(scene)
    fops = [FittingOP({}, {}, N, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid, camera_ext=cam, dct_mtx=D, c_dct_init=c0[k])
            for k, (_, cam) in enumerate(clips)]
    bodies = [torch.tensor(body).cuda() for body, _ in clips]
    num_iter = DCT_NUM_ITER
    P = dct_first_phase2_iter(num_iter)

    def batch(K):
        t0 = time.perf_counter()
        r = [(b.cpu(), s, c.cpu()) for b, s, c in fitter.fit(clips[:K], mode="dct", dct_mtx=D, c_dct_init=c0[:K])]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def alone(K):
        t0 = time.perf_counter()
        r = []
        for k in range(K):
            b, s, c = fops[k].fitting(bodies[k], "dct")
            r.append((b.cpu(), s, c.cpu()))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def phases(K):
        """the batch's first and second phase, each one fdcap_opt_run_dct stretch between two events (ms)"""
        fitter.prepare(clips[:K], "dct")
        lib, h, st = fitter.ctx.lib, fitter.ctx.handle, capi.current_stream()
        cd = torch.cat([torch.tensor(a) for a in c0[:K]]).cuda().contiguous()
        capi.check(lib.fdcap_opt_set_dct_clips(h, D.ctypes.data_as(ctypes.c_void_p), D.shape[0], D.shape[1], capi.dptr(cd), st), "set_dct_clips")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        n = ctypes.c_int32(0)
        wd, wr, wc = DCT_PHASE2
        ev[0].record()
        capi.check(lib.fdcap_opt_run_dct(h, 0, P, num_iter, DCT_PHASE1_WEIGHT, wd, wr, wc, 0, None, None, 0, 0, ctypes.byref(n), st), "run_dct")
        ev[1].record()
        capi.check(lib.fdcap_opt_run_dct(h, P, num_iter, num_iter, DCT_PHASE1_WEIGHT, wd, wr, wc, 0, None, None, 0, 0, ctypes.byref(n), st), "run_dct")
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])

    res = {"problem": {"verts": 10475, "contacts": len(vid), "scene": NS, "frames_per_clip": N, "iters": num_iter, "first_phase_iters": P,
                       "second_phase_iters": num_iter - P - 1, "mode": "dct", "reps": reps}, "sweep": []}
    for K in ks:
        _, rb = batch(K)
        _, ra = alone(K)
        worst = max(float((b[0] - a[0]).abs().max()) for b, a in zip(rb, ra))
        tb, ta = [], []
        for _ in range(reps):
            tb.append(batch(K)[0])
            ta.append(alone(K)[0])
        ph = [phases(K) for _ in range(reps)]
        p1, p2 = float(np.median([p[0] for p in ph])), float(np.median([p[1] for p in ph]))
        mb, ma = float(np.median(tb)), float(np.median(ta))
        res["sweep"].append({"K": K, "rows": K * N, "trajectory_waves": K * (N // 60) * 69, "batch_ms": mb * 1e3,
                             "batch_ms_all": [t * 1e3 for t in tb], "stand_alone_ms": ma * 1e3, "stand_alone_ms_all": [t * 1e3 for t in ta],
                             "batch_clips_per_s": K / mb, "stand_alone_clips_per_s": K / ma, "batch_over_stand_alone": ma / mb,
                             "batch_first_phase_ms": p1, "batch_second_phase_ms": p2, "first_phase_us_per_iter": p1 * 1e3 / P,
                             "second_phase_us_per_iter": p2 * 1e3 / max(num_iter - P - 1, 1), "max_abs_body_difference": worst})
        print(f"K {K}: batch {mb * 1e3:8.2f} ms ({K / mb:6.2f} clips/s)  stand-alone x{K} {ma * 1e3:8.2f} ms ({K / ma:6.2f} clips/s)  "
              f"ratio {ma / mb:5.2f}  phases {p1:7.2f} + {p2:7.2f} ms ({p1 * 1e3 / P:5.2f} us per first-phase iteration)", file=sys.stderr, flush=True)
    fitter.close()
    for f in fops:
        f.close()
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
