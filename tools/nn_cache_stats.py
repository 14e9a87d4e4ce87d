#!/usr/bin/env python3
"""Work-list cache of the in-loop NN launch over a whole fit: kept / rebuilt waves and list sizes per block of iterations.
BOX_HIST=<block> (r15): instead, per block of that many launches, the count n that enters each of the search's three box-test stages
(near chunks of a batch, 4 x listed chunks, the filter's raw list): stages run, mean and largest n, shares n <= 8 / <= 16 / <= 32.
ITEMS=<block> (r21): instead, per block of that many launches and per wave: listed items (the raw list the filter takes), scanned items
(after the filter), 32-point tiles scored and tiles with a filter hit.  KEY_SHIFT=<5|6|7> forces the query order's key
and ITEMS_PER_CHUNK=<4|8> its work items (fdcap_debug_nn_search_form; default: the build's own choice).
Needs the -DFDC_NN_STATS build (FDCAP_LIB)."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import fdcap_amd  # noqa
from fdcap_amd import capi, synth
from fdcap_amd.fitting import FittingOP, first_phase2_iter
from fdcap_amd.io import read_camerapose
C5 = os.environ.get("CONFIG") == "c5"                       # r6: BASELINE config 5 (512 frames, 2 M points, every vertex a contact)
N, ns = int(os.environ.get("FRAMES", "512" if C5 else "1024")), (2000000 if C5 else 500000)
bm = synth.make_body_model(10475, seed=0); vp = synth.make_vposer(seed=1); clip = synth.make_clip(N, seed=3)
scene = synth.make_scene(ns, seed=2); l, r = synth.make_contact_ids(bm.v_template, per_part=250, seed=4)
if C5: l, r = np.arange(0, 5237), np.arange(5237, 10475)
fop = FittingOP({"num_iter": 500}, {}, N, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=np.concatenate([l, r]),
                camera_ext=read_camerapose(clip.camerapose_lines))
lib, h = fop.ctx.lib, fop.ctx.handle
raw = ctypes.CDLL(capi.LIB_PATH)
raw.fdcap_debug_nn_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]
body = torch.tensor(clip.body_params).cuda()
x78 = torch.empty(N, capi.XDIM, device="cuda")
capi.check(lib.fdcap_params_75_to_78(capi.dptr(body), N, capi.dptr(x78), capi.current_stream()), "75->78")
fop._mode = "global"; fop.init(x78)
P = first_phase2_iter(500)
if os.environ.get("KEY_SHIFT") or os.environ.get("ITEMS_PER_CHUNK"):
    capi.check(lib.fdcap_debug_nn_search_form(h, int(os.environ.get("KEY_SHIFT", "0")), int(os.environ.get("ITEMS_PER_CHUNK", "0"))), "nn_search_form")
ITEMS = int(os.environ.get("ITEMS", "0"))
out = (ctypes.c_ulonglong * 8)()
raw.fdcap_debug_nn_stats(out)
BOX = int(os.environ.get("BOX_HIST", "0"))
box = (ctypes.c_ulonglong * 18)()
if BOX: raw.fdcap_debug_nn_box_hist.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]; raw.fdcap_debug_nn_box_hist(box)
for ii in range(P):
    st = capi.current_stream()
    capi.check(lib.fdcap_opt_backward(h, ii, P, 0, st), "bwd"); capi.check(lib.fdcap_opt_step(h, ii, P, st), "step")
    if ITEMS:
        if ii % ITEMS == ITEMS - 1 or ii == P - 1:
            raw.fdcap_debug_nn_stats(out)
            w = max(out[4] + out[5], 1)
            print(f"launches {ii - ii % ITEMS:3d}-{ii:3d}: per wave listed {out[6] / w:5.2f}  scanned {out[3] / w:5.2f}  tiles {out[0] / w:5.2f}  "
                  f"tiles with a hit {out[1] / w:5.2f}  (lists kept {out[4] / w:6.1%})")
        continue
    if BOX:
        if ii % BOX == BOX - 1 or ii == P - 1:
            raw.fdcap_debug_nn_box_hist(box)
            print(f"launches {ii - ii % BOX:3d}-{ii:3d}")
            for s, name in enumerate(("near chunks per batch", "4 x listed chunks", "filter n_raw")):
                b = list(box[6 * s:6 * s + 6]); tot = max(sum(b[:4]), 1)
                print(f"   {name:22s} stages {sum(b[:4]):9d}  mean n {b[4] / tot:6.2f}  max {b[5]:4d}  n<=8 {b[0] / tot:6.1%}  n<=16 {(b[0] + b[1]) / tot:6.1%}"
                      f"  n<=32 {(b[0] + b[1] + b[2]) / tot:6.1%}")
        continue
    if ii % 25 == 24 or ii < 3:
        raw.fdcap_debug_nn_stats(out)
        kept, built, rawn, filt, items, mf = out[4], out[5], out[6], out[7], out[3], out[0]
        w = max(kept + built, 1)
        hb = (ctypes.c_ulonglong * 96)(); raw.fdcap_debug_nn_hist(hb)
        if ii % 100 == 99 or ii < 1:
            print("   slow-path entries per wave (log2 buckets):", list(hb[32:48]))
            print("   longest per-lane exact chain per wave (log2 buckets):", list(hb[64:80]))
            print("   work items per wave, log2 buckets [0,1,2-3,4-7,8-15,16-31,32-63,...]: listed", list(hb[:12]), " overflowed", list(hb[16:30]))
        print(f"iter {ii:3d}: kept {kept/w:6.1%}  raw list {rawn/w:5.1f}  after filter {filt/w:5.1f}  work items {items/w:5.1f}  MFMA results/wave {mf/w:5.1f}")
