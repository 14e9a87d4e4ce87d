"""The device build of csrc/fdc_math.h at the rest pose, tiny angles, half turns, every quaternion branch and deformed 6D codes:
tests/rotation_edges.py's tables and bars (32 x max(fp32 oracle - fp64 oracle, 2^-24 max|value|), per group / joint / frame, from
the oracle's two precisions; tests/test_rotation_edges_cpu.py shows that the host build is inside them and seven defects are not)
through every kernel that calls the five conversions outside the timed loop, and through the loop's backward at a half-turn clip.

Worst measured max|err| / bar on the MI355X (every case was inside its bar at the first run; the only defect these cases found was in
Python: ops.BodyModel read the batch size from body_pose and raised when it was left None):
  75 -> 78 (B = table and B = 1, same bits)   rest 0   tiny 0.031   near_half 0.031   exact_half 0.042   quarter 0.021   branches 0.046
                                              generic 0.027
  78 -> 75                                    exact: rest 0 (exactly 0), tiny 0.034, near_half 0.031, quarter 7e-10, branches 0.033,
                                              generic 0.033, exact_half 0.086 (rotation space)   scaled: near_half 0.048, generic
                                              0.049, exact_half 0.127   sheared: near_half 0.073, generic 0.041, exact_half 0.086
                                              parallel: near_half 0.064, generic 0.036, exact_half 0.050   identity 0 (exactly 0)
  vposer decode, outputs / d z                edges: aa 0.066 / 0.0098, matrot 0.090 / 0.012   deformed: aa 0.23 / 0.067, matrot
                                              0.14 / 0.024   half: aa 0.12 / 0.042, matrot 0.10 / 0.033   branches: aa 0.11 / 0.018,
                                              matrot 0.065 / 0.019   identity: aa 0.087 / 0.016, matrot 0.091 / 0.020 (joint 0:
                                              aa = 0 and R = I exactly, d z finite)
  body model, vertices / joints / worst gradient
                                              rest 0.022 / 0.039 / 0.11 (transl)   tiny 0.049 / 0.034 / 0.13 (left hand)   near_half
                                              0.11 / 0.041 / 0.32 (right hand; global_orient 0.22)   exact_half 0.064 / 0.063 / 0.12
                                              pi_x 0.052 / 0.031 / 0.058   rest_jaw0 0.019 / 0.044 / 0.080 (jaw 0.056)   jaw_zero
                                              0.034 / 0.047 / 0.050 (jaw 0.020)   jaw_tiny 0.045 / 0.043 / 0.13 (jaw 0.044)   jaw_half
                                              0.046 / 0.043 / 0.11 (jaw 0.089)
  flip, once / twice                          rest 0.031 / 0.031   yaw 0.098 / 0.098   pi_x 0.031 / 0.063   exact_half 0.052 / 0.063
  half-turn clip, contact term                transl 0.034   sixd 0.020   betas 0.018   latent 0.011   lh 0.011   rh 0.014   camt 0.029
                                              dscale 0.015
  half-turn clip, world term                  transl 0.066   sixd 0.045   betas 0.0099   latent 0.018   lh, rh 0 (exact zeros)
                                              camt 0.031   cam_rot 0.031   cam_transl 0.031   cam_bottom 0 (exact zeros)"""
import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
import tests.gradient_bars as gb
from fdcap_amd import capi, ops, synth
from tests import rotation_edges as re_

pytestmark = pytest.mark.gpu


def _dev(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float32).cuda().requires_grad_(grad)


# ---- fdcap_params_75_to_78 / fdcap_params_78_to_75 --------------------------------------------------------------------------------------------
def _convert(fn, x, width, batched):
    lib = capi.load_library()
    x = _dev(x)
    n = x.shape[0]
    if batched:
        out = torch.full((n, width), float("nan"), device="cuda")
        capi.check(fn(lib)(capi.dptr(x), n, capi.dptr(out), capi.current_stream()), "conversion")
    else:
        rows = [torch.full((1, width), float("nan"), device="cuda") for _ in range(n)]
        for i in range(n):
            capi.check(fn(lib)(capi.dptr(x[i:i + 1].contiguous()), 1, capi.dptr(rows[i]), capi.current_stream()), "conversion")
        out = torch.cat(rows)
    return out.cpu().numpy()


@pytest.mark.parametrize("batched", [True, False], ids=["B=table", "B=1"])
def test_param_conversions_at_the_edges(batched):
    """p75_to_78_kernel on the whole axis-angle table (columns 3:6), p78_to_75_kernel on the whole 6D table (columns 3:9), in one
    launch and row by row: every group inside its bar (the exact_half rows of 78 -> 75 in rotation space, all others vector against
    vector), the other 72 columns bit for bit."""
    x75, x78 = re_.x75_rows(), re_.x78_rows()
    got78 = _convert(lambda lib: lib.fdcap_params_75_to_78, x75, 78, batched)
    got75 = _convert(lambda lib: lib.fdcap_params_78_to_75, x78, 75, batched)
    assert np.array_equal(np.delete(got78, np.s_[3:9], 1).view(np.uint32), np.delete(x75.astype(np.float32), np.s_[3:6], 1).view(np.uint32))
    assert np.array_equal(np.delete(got75, np.s_[3:6], 1).view(np.uint32), np.delete(x78.astype(np.float32), np.s_[3:9], 1).view(np.uint32))
    bad = {"75->78": re_.check_conversion("aa_to_sixd", got78[:, 3:9], "device 75 -> 78"),
           "78->75": re_.check_conversion("sixd_to_aa", got75[:, 3:6], "device 78 -> 75")}
    assert not any(bad.values()), bad


# ---- fdcap_vposer_decode / fdcap_vposer_decode_bwd --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decoders():
    bm = synth.make_body_model(120, seed=0)
    ctxs = {name: capi.Context(bm, re_.vposer_data(synth.make_vposer(seed=1), name)) for name in re_.vposer_joint_codes()}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("output_type", ["aa", "matrot"])
@pytest.mark.parametrize("context", list(re_.vposer_joint_codes()))
def test_vposer_decode_and_backward_with_every_joint_at_an_edge(decoders, context, output_type, B):
    """sixd_to_rot_kernel and vposer_out_bwd_kernel (gs_forward / gs_backward, tgm_rotmat_to_aa and its backward) with the 21
    joints' output bias at chosen codes of the 6D table: outputs per joint, d z per context.  `identity`: joint 0 sits at R == I
    exactly (zero output weights), where the backward takes the s2 == 0 branch -- its gradient must be finite (a NaN there would
    reach every element of d z through 0 x NaN) and d z must be what the oracle gives with that joint continued from 1e-4 rad; the
    VALUE of that branch cannot be seen through d z (the joint's weights are zero, and any code that is exactly the identity for
    some z has a zero derivative in z): it is pinned on the host build (tests/test_rotation_edges_cpu.py)."""
    case = re_.vposer_case(context, output_type, B)
    z = _dev(case["z"], True)
    out = ops.VPoser(decoders[context]).decode(z, output_type=output_type).reshape(B, 21, -1)
    (out * _dev(case["w"])).sum().backward()
    got, dz = out.detach().cpu().numpy(), z.grad.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(dz).all()
    if context == "identity":
        want = np.zeros(3) if output_type == "aa" else np.eye(3).reshape(9)
        assert np.array_equal(got[:, 0], np.tile(want, (B, 1)))
    bad = re_.check_vposer(case, got, dz, f"device vposer {context} {output_type} B = {B}")
    assert not bad, bad


# ---- ops.BodyModel ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def body_ctx():
    ctx = capi.Context(synth.make_body_model(120, seed=0), synth.make_vposer(seed=1))
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name", list(re_.body_poses()))
def test_body_model_forward_and_backward_at_edge_poses(body_ctx, name):
    """assemble_rows_kernel, the axis-angle path of pose_fwd_kernel, pose_bwd_op_kernel and the skinning chain (rodrigues_forward /
    rodrigues_backward) at the rest pose (every pose argument None), every tiny theta, near and exact half turns for global_orient and
    all 21 body joints, global_orient = (pi, 0, 0), and the face operator's jaw at 0, tiny thetas and next to pi: vertices, joints and
    the gradient of every given input, per frame, finite and inside the bars; Rodrigues is smooth through pi, so every row is compared
    directly."""
    case = re_.body_case(name)
    g = {k: _dev(v, True) for k, v in case["inputs"].items() if v is not None}
    out = ops.BodyModel(body_ctx)(return_verts=True, **g)
    ((out.vertices * _dev(case["wv"])).sum() + (out.joints * _dev(case["wj"])).sum()).backward()
    grads = {k: v.grad.cpu().numpy() for k, v in g.items()}
    assert all(np.isfinite(a).all() for a in grads.values())
    bad = re_.check_body(case, out.vertices.detach().cpu().numpy(), out.joints.detach().cpu().numpy(), grads, f"device body model {name}")
    assert not bad, bad


# ---- fdcap_fit2d_flip_orient -----------------------------------------------------------------------------------------------------------------
def test_flip_at_rest_yaw_and_half_turns():
    """fit2d_flip_kernel (rodrigues_forward, then tgm_rotmat_to_aa off the trace branch) on aa = 0, pure yaw up to pi, (pi, 0, 0),
    (pi - 1e-3, 0, 0) and the exact_half axes, against fit2d_init_spec.flip_rotation in rotation space; flipped twice against the
    rotation itself, in rotation space as well (at a half turn the vector may come back negated)."""
    c = re_.flip_case()
    n = len(c["aa"])
    rows = np.random.default_rng(50).standard_normal((n, 75)).astype(np.float32)
    rows[:, 3:6] = c["aa"]
    d = torch.tensor(rows).cuda()
    lib = capi.load_library()
    capi.check(lib.fdcap_fit2d_flip_orient(capi.dptr(d), n, capi.current_stream()), "flip")
    once = d.cpu().numpy()
    capi.check(lib.fdcap_fit2d_flip_orient(capi.dptr(d), n, capi.current_stream()), "flip")
    twice = d.cpu().numpy()
    keep = [k for k in range(75) if not 3 <= k < 6]
    assert np.array_equal(once[:, keep].view(np.uint32), rows[:, keep].view(np.uint32)) and np.array_equal(twice[:, keep].view(np.uint32), rows[:, keep].view(np.uint32))
    assert np.isfinite(once).all() and np.isfinite(twice).all()
    r1 = re_.group_ratios(re_.rodrigues64(once[:, 3:6]), c["once64"], c["bar_once"], c["group"])
    r2 = re_.group_ratios(re_.rodrigues64(twice[:, 3:6]), c["twice64"], c["bar_twice"], c["group"])
    re_.show("device flip once", r1)
    re_.show("device flip twice", r2)
    assert max(np.linalg.norm(once[:, 3:6], axis=1).max(), np.linalg.norm(twice[:, 3:6], axis=1).max()) <= re_.PI + 1e-5
    assert not re_.outside(r1) and not re_.outside(r2), (re_.outside(r1), re_.outside(r2))


# ---- the loop's backward at a half-turn clip -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("term", ["con", "ws"])
def test_isolated_terms_at_a_half_turn_clip(term):
    """fdcap_opt_backward (gs_forward / gs_backward on the optimiser's path) on the smallest parity case with every global_orient
    composed with (pi, 0, 0) and the root 6D columns of two frames scaled and sheared (rotation_edges.HalfTurnClip): the isolated
    contact term and the isolated world term, every block within its bar from the oracle at the state the device holds."""
    from tests.test_gpu_gradient_bars import isolated_backward
    it = gb.isolated_terms(re_.HALF_TURN_CASE, re_.HalfTurnClip)
    got, _ = isolated_backward(re_.HALF_TURN_CASE, term, it)
    assert all(np.isfinite(v).all() for v in got.values())
    bad = gb.check(got, it["g64"][term], it["bar"][term], gb.COEFF[term], f"half-turn clip {re_.HALF_TURN_CASE} {term}")
    assert not bad, f"blocks outside their bar {{block: (err / bar, bar, max|g|)}}: {bad}"
