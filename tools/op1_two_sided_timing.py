#!/usr/bin/env python3
"""Op 1 as a two-sided operator: milliseconds per forward + backward of ops.chamferDist(both=True) with BOTH inputs requiring
grad (HIP events around windows of ITERS calls, after warm-up; median and range over REPEATS windows), and for the shared-target
case the peak device memory of one forward + backward.  Cases:
    per-batch targets   B in {1, 64, 1024} x (n, m) = (500, 10475)     -- a body <-> body / body <-> scan Chamfer over a clip
    shared [1,m,3]      (B, n, m) = (256, 500, 100000)                 -- the target's gradient summed over the batch
Runs on any commit that has ops.chamferDist: `python3 tools/op1_two_sided_timing.py [label]`.  Development tool
(profiles/op1_two_sided_timing.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import fdcap_amd  # noqa
from fdcap_amd import capi, ops, synth

LABEL = sys.argv[1] if len(sys.argv) > 1 else "this commit"
REPEATS = int(os.environ.get("REPEATS", 5))
CASES = [(1, 500, 10475, False, 300), (64, 500, 10475, False, 40), (1024, 500, 10475, False, 3), (256, 500, 100_000, True, 5)]

assert torch.cuda.is_available(), "needs the GPU: a CPU run cannot give a time"
ctx = capi.Context(synth.make_body_model(300, seed=0), synth.make_vposer(seed=1))
op = ops.chamferDist(ctx, both=True, use_registered_scene=False)


def once(x1, x2, w1, w2):
    x1.grad = x2.grad = None
    d1, d2 = op(x1, x2)
    ((d1 * w1).sum() + (d2 * w2).sum()).backward()


print(f"# {LABEL}: ops.chamferDist(both=True), forward + backward, both inputs require grad; {REPEATS} windows per case")
for B, n, m, shared, iters in CASES:
    rng = np.random.default_rng(1000 * B + n + m)
    x1 = torch.tensor(rng.uniform(-1, 1, size=(B, n, 3)).astype(np.float32), device="cuda").requires_grad_(True)
    x2 = torch.tensor(rng.uniform(-1, 1, size=(1 if shared else B, m, 3)).astype(np.float32), device="cuda").requires_grad_(True)
    w1, w2 = torch.randn(B, n, device="cuda"), torch.randn(B, m, device="cuda")
    for _ in range(2):
        once(x1, x2, w1, w2)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    once(x1, x2, w1, w2)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ms = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            once(x1, x2, w1, w2)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    ms.sort()
    kind = "shared [1,m,3]" if shared else "per-batch"
    print(f"{LABEL:12s} B={B:5d} n={n} m={m:6d} {kind:15s} {ms[len(ms) // 2]:10.3f} ms  (min {ms[0]:.3f}, max {ms[-1]:.3f}; {iters} calls per window)"
          f"  peak torch memory above the inputs {peak / 2**20:9.1f} MiB  grad2 {tuple(x2.grad.shape)}", flush=True)
    del x1, x2, w1, w2
    torch.cuda.empty_cache()
ctx.close()
