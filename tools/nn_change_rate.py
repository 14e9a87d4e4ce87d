#!/usr/bin/env python3
"""How many neighbour records does a launch of the in-loop search really change?  (r14: what not rewriting the unchanged ones can
save at most.)  One fit of the bench workload (BASELINE config 3: 1024 frames, 500 contacts, 500 k scene points); after every
phase-1 iteration the search's idx is read back and compared with the iteration before.  Per block of 50 launches: the share of
queries whose neighbour changed, and the share of the 128-byte lines of idx (32 queries) and of seedpt (8 queries) that hold at
least one changed query -- a line with one changed record is written back whole.  Queries are taken in the library's own memory
order: frame-major, the contacts of a frame in the library's slot order (fdcap_debug_contact_perm), both arrays offset by the two
guard rows in front of the clip.
   python tools/nn_change_rate.py [--frames 1024] [--scene 500000] [--iters 500] [--out profiles/r14_nn_change_rate.txt]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import fdcap_amd  # noqa
from fdcap_amd import capi, synth
from fdcap_amd.fitting import FittingOP, first_phase2_iter
from fdcap_amd.io import read_camerapose

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1024)
ap.add_argument("--scene", type=int, default=500_000)
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--out", default=None)
a = ap.parse_args()
N = a.frames
bm = synth.make_body_model(10475, seed=0); vp = synth.make_vposer(seed=1); clip = synth.make_clip(N, seed=3)
scene = synth.make_scene(a.scene, seed=2); l, r = synth.make_contact_ids(bm.v_template, per_part=250, seed=4)
ids = np.concatenate([l, r]); nc = len(ids)


fop = FittingOP({"num_iter": a.iters}, {}, N, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=ids,
                camera_ext=read_camerapose(clip.camerapose_lines))
perm_h = np.empty(nc, dtype=np.int32)                                     # slot -> position in the caller's id array, from the library
capi.check(fop.ctx.lib.fdcap_debug_contact_perm(fop.ctx.handle, perm_h.ctypes.data, nc), "fdcap_debug_contact_perm")
assert sorted(perm_h.tolist()) == list(range(nc))
perm = torch.tensor(perm_h.astype(np.int64), device="cuda")
P = first_phase2_iter(a.iters)
q = torch.arange(N * nc, device="cuda") + 2 * nc                          # element offset of query q in idx / seedpt
line_i, line_p = q // 32, q // 8
nli, nlp = int(line_i.max() - line_i.min()) + 1, int(line_p.max() - line_p.min()) + 1
line_i -= line_i.min(); line_p -= line_p.min()
prev = [None]
rows = []                                                                  # per launch: (changed queries, dirty idx lines, dirty seedpt lines)


def hook(k):
    # after step k: the search of iteration k - 1
    idx = torch.empty(N, nc, dtype=torch.int32, device="cuda")
    capi.check(fop.ctx.lib.fdcap_opt_get_contact(fop.ctx.handle, None, capi.dptr(idx), capi.current_stream()), "get_contact")
    cur = idx[:, perm].reshape(-1)
    if prev[0] is not None:
        ch = cur != prev[0]
        di = torch.zeros(nli, dtype=torch.bool, device="cuda"); di[line_i[ch]] = True
        dp = torch.zeros(nlp, dtype=torch.bool, device="cuda"); dp[line_p[ch]] = True
        rows.append((k - 1, float(ch.float().mean()), float(di.float().mean()), float(dp.float().mean())))
    prev[0] = cur.clone()


fop.snapshot_hook = hook
fop.fitting(torch.tensor(clip.body_params).cuda(), "global", log_every=0, snapshot_at=range(1, P + 1))
lines = [f"# tools/nn_change_rate.py: {N} frames x {nc} contacts = {N * nc} queries, {a.scene} scene points, {P} phase-1 launches",
         "# launches: changed queries | 128-byte lines of idx with a changed query | of seedpt   (shares, mean over the block)"]
R = np.array(rows)
for b0 in range(0, len(R), 50):
    blk = R[b0:b0 + 50]
    lines.append(f"{int(blk[0, 0]):4d}-{int(blk[-1, 0]):4d}: {blk[:, 1].mean():.4f} | {blk[:, 2].mean():.4f} | {blk[:, 3].mean():.4f}")
lines.append(f"all      : {R[:, 1].mean():.4f} | {R[:, 2].mean():.4f} | {R[:, 3].mean():.4f}")
mb_i, mb_p = N * nc * 4 / 1e6, N * nc * 16 / 1e6
lines.append(f"# bytes a launch need not write (mean): idx {mb_i * (1 - R[:, 2].mean()):.2f} of {mb_i:.2f} MB, seedpt "
             f"{mb_p * (1 - R[:, 3].mean()):.2f} of {mb_p:.2f} MB")
print("\n".join(lines))
if a.out:
    with open(a.out, "w") as f: f.write("\n".join(lines) + "\n")
