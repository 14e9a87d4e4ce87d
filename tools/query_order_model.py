#!/usr/bin/env python3
"""CPU model of which queries should share a wave of the in-loop search (NOTES "Round 7"): the quarters of the k-d order
(tests/scene_spec.py) that each group of 32 queries reaches with its exact neighbour distance as the bound, for 32 consecutive query
indices against groups sorted by the quarter of each query's neighbour.  Queries: the contact vertices of the bench clip's STARTING
state (the oracle's forward; a converged fit needs the GPU).
   python tools/query_order_model.py [frames=1024] [scene points=500000] [all]"""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import fdcap_amd  # noqa
from fdcap_amd import synth
from oracle import rotrepr
from oracle.fitting import FittingOracle
from oracle.smplx import SMPLXOracle
from oracle.vposer import VPoserDecoder
import scene_spec as ss
from scipy.spatial import cKDTree
F = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
NS = int(sys.argv[2]) if len(sys.argv) > 2 else 500_000
ALLC = len(sys.argv) > 3 and sys.argv[3] == "all"
t0 = time.time()
bm = synth.make_body_model(10475, seed=0, lbs_nnz=4)
vp = synth.make_vposer(seed=1)
clip = synth.make_clip(F, seed=3)
scene = synth.make_scene(NS, seed=2)
left, right = synth.make_contact_ids(bm.v_template, per_part=250, seed=4)
vid = np.arange(10475) if ALLC else np.concatenate([left, right])
torch.set_num_threads(8)
f = FittingOracle(SMPLXOracle(bm), VPoserDecoder.from_data(vp), scene[:10], vid, clip.camerapose_lines[:F], F, num_iter=10)
x78 = rotrepr.convert_to_6D_rot(torch.tensor(clip.body_params[:F]))
f.init(x78)
with torch.no_grad():
    _, verts, _ = f.forward_world()
Q = verts[:, vid, :].reshape(-1, 3).numpy().astype(np.float32)
nq = Q.shape[0]
print("queries", Q.shape, "t", time.time() - t0, flush=True)
order = ss.order_spec(scene)
t = ss.tables_spec(scene, order)
srt = t["sorted"][:, :3]
qb = t["qbounds"].reshape(-1, 2, 4)[:, :, :3]   # [nquarter, 2, 3]
print("tables t", time.time() - t0, flush=True)
tree = cKDTree(srt)
d, pos = tree.query(Q, k=1)
d2 = d.astype(np.float64) ** 2
print("median radius", np.median(d), "t", time.time() - t0, flush=True)
# quarters reached per query: quarter box within the ball (box distance^2 <= d2)
qcen = 0.5 * (qb[:, 0] + qb[:, 1]); qhalf = 0.5 * (qb[:, 1] - qb[:, 0])
valid = np.isfinite(qcen).all(1)
qcen, qhalf = np.where(valid[:, None], qcen, 1e9), np.where(valid[:, None], qhalf, 0)
qtree = cKDTree(qcen)
maxhalf = np.linalg.norm(qhalf, axis=1).max()
reach = [None] * nq
for i in range(nq):
    cand = qtree.query_ball_point(Q[i], d[i] + maxhalf + 1e-6)
    cand = np.asarray(cand, dtype=np.int64)
    dd = np.maximum(np.abs(Q[i] - qcen[cand]) - qhalf[cand], 0)
    reach[i] = cand[(dd * dd).sum(1) <= d2[i] * 1.00002 + 1e-9]
print("reach t", time.time() - t0, "mean per query", np.mean([len(r) for r in reach]), flush=True)
def per_group(perm):
    tot = []
    for g0 in range(0, nq, 32):
        s = set()
        for q in perm[g0:g0 + 32]:
            s.update(reach[q].tolist())
        tot.append(len(s))
    return np.array(tot)
ident = np.arange(nq)
key_q = pos >> 7
lb = np.clip(np.floor(np.log2(np.maximum(d, 1e-6) / 1e-3) * 2), 0, 31).astype(np.int64)  # half-octave buckets from 1 mm
forms = {
    "identity": ident,
    "quarter>>7, logdist, index": np.lexsort((ident, lb, key_q)),
    "quarter>>7, index": np.lexsort((ident, key_q)),
    "logdist, quarter>>7, index": np.lexsort((ident, key_q, lb)),
}
for name, p in forms.items():
    g = per_group(p)
    print(f"{name:32s} quarters/group mean {g.mean():7.2f}  tiles {4*g.mean():7.2f}  p50 {np.median(g):.0f} p90 {np.percentile(g,90):.0f}", flush=True)
