"""tests/rotation_edges.py without a GPU: the conditions its bars rest on (the oracle alone), the host build of csrc/fdc_math.h inside
every bar, and every mutant outside by a factor.

The host build (g++, -ffp-contract=off, libm) passing here says nothing about the device build (-O3, contraction, ocml,
-fno-honor-nans): tests/test_gpu_rotation_edges.py runs the same table and the same bars through the kernels."""
import ctypes

import numpy as np
import pytest

import fdcap_amd  # noqa: F401
from fdcap_amd import synth
from tests import host_pipeline, rotation_edges as re_
from tests.host_pipeline import HostPipeline, P

MIN_FACTOR = 2.0


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


@pytest.fixture(scope="module")
def lib():
    return host_pipeline.build()


def _call(fn, out_shape, *arrays):
    """fn(*arrays as float*, n, out) -> out [n, ...] (fp32)"""
    ins = [f32(a) for a in arrays]
    out = np.zeros(out_shape, np.float32)
    fn(*[P(a) for a in ins], ctypes.c_int(out_shape[0]), P(out))
    return out


# ---- the reference alone ----------------------------------------------------------------------------------------------------------------
def test_table_holds_every_branch_and_the_oracles_agree_off_the_excused_rows():
    """The branch counts (from the fp64 rotation, as tests/test_host_math.py counts them), finite oracle values wherever a bar is
    formed from them, and direct fp32 / fp64 agreement of R -> aa on every row that is not excused: the cap on excused rows holds
    for the reference alone."""
    aa, group = re_.aa_table()
    br = re_.quaternion_branch(re_.rodrigues64(aa))
    for k in range(4):
        assert np.array_equal(br[group == f"branches:{k}"], np.full(re_.PER_BRANCH, k)) and re_.PER_BRANCH >= 8, k
    counts = np.bincount(br, minlength=4)
    print("rows per quaternion branch over the whole table:", counts.tolist())
    assert counts.min() >= 8
    th2 = (aa * aa).sum(1)
    assert (th2[np.char.startswith(group, "tiny")] <= 1e-6).sum() >= 9 and (th2[np.char.startswith(group, "tiny")] > 1e-6).sum() >= 9
    s, g6, src = re_.sixd_table()
    a1, a2 = s[:, 0::2], s[:, 1::2]
    cos = (a1 * a2).sum(1) / np.linalg.norm(a1, axis=1) / np.linalg.norm(a2, axis=1)
    assert np.allclose(cos[np.char.startswith(g6, "sheared")], 0.9, atol=1e-6) and np.allclose(cos[np.char.startswith(g6, "parallel")], 0.9998, atol=1e-6)
    assert np.array_equal(s[g6 == "identity"][0], [1, 0, 0, 1, 0, 0])
    c = re_.conversions()
    for name, e in c.items():
        assert np.isfinite(e["o64"]).all() and np.isfinite(e["o32"]).all(), name
        assert all(np.isfinite(b) for b in e["bar"].values()), name
    assert c["rotmat_to_aa_bwd"]["at_identity"].tolist() == np.nonzero(group == "rest")[0].tolist()
    for name in ("sixd_to_aa", "rotmat_to_aa"):
        e = c[name]
        ex = e["excused"]
        assert ex.sum() == (12 if name == "rotmat_to_aa" else 48), ex.sum()                    # fixed by the table
        d = np.abs(e["o32"][~ex] - e["o64"][~ex]).max()
        print(f"{name}: fp32 / fp64 oracle, max direct difference off the {ex.sum()} excused rows {d:.3g}")
        assert d <= re_.DIRECT_AGREEMENT
        assert np.abs(re_.rodrigues64(e["o64"]) - e["R64"]).max() <= 1e-6                       # (fp32-rounded R is off SO(3) by 6e-8)
        assert (np.linalg.norm(e["o64"], axis=1) <= re_.PI + 1e-12).all()


@pytest.mark.parametrize("name", list(re_.MUTANTS))
def test_every_mutant_leaves_the_bars(name):
    """Not covered: none -- every mutant of the list is outside its entry point's bars by the factor printed here.  (trace_only is a loss
    of precision, not another function: evaluated in fp32, as a kernel would compute it; see rotation_edges.MUTANTS.)"""
    factor, where = re_.mutant_factor(name)
    print(f"mutant {name}: outside its bar by a factor {factor:.3g} at {where}")
    assert factor >= MIN_FACTOR


def test_vposer_mutants_are_seen_through_the_decoder():
    """The decoder-level bars (per joint, d z per context) see the same defects: the nearly parallel and half-turn joints do not hide
    the others."""
    import torch
    from oracle import rotrepr
    from oracle.vposer import VPoserDecoder

    def run(case, output_type, gs_fn=rotrepr.decode_6d, aa_fn=rotrepr.matrot2aa):
        B = case["z"].shape[0]
        z = torch.tensor(case["z"], dtype=torch.float64, requires_grad=True)
        dec = VPoserDecoder.from_data(case["vp"], torch.float64)
        h = torch.nn.functional.leaky_relu(torch.nn.functional.linear(z, dec.fc1_w, dec.fc1_b), 0.2)
        h = torch.nn.functional.leaky_relu(torch.nn.functional.linear(h, dec.fc2_w, dec.fc2_b), 0.2)
        out = gs_fn(torch.nn.functional.linear(h, dec.out_w, dec.out_b))
        out = aa_fn(out) if output_type == "aa" else out
        out = out.reshape(B, 21, -1)
        (out * torch.tensor(case["w"])).sum().backward()
        return out.detach().numpy(), z.grad.numpy()

    for context, output_type, kw, what in (("deformed", "matrot", dict(gs_fn=re_._m_gs_no_ddu), "dz"),
                                           ("edges", "aa", dict(aa_fn=re_._m_no_qw_rule), "out"),
                                           ("deformed", "aa", dict(aa_fn=re_._m_no_qw_rule), "out"),
                                           ("half", "aa", dict(aa_fn=re_._m_no_qw_rule), "dz")):
        case = re_.vposer_case(context, output_type, 5)
        assert not re_.check_vposer(case, *run(case, output_type), f"oracle fp64 {context} {output_type}")
        out = re_.check_vposer(case, *run(case, output_type, **kw), f"mutant {list(kw.values())[0].__name__} {context} {output_type}")
        worst = max(v for k, v in out.items() if (k == "dz") == (what == "dz")) if out else 0.0
        assert worst >= MIN_FACTOR, (context, output_type, out)


# ---- the host build inside the bars -----------------------------------------------------------------------------------------------------
def test_host_conversions_inside_the_bars(lib):
    """tgm_aa_to_rotmat (75 -> 78), gs_forward + tgm_rotmat_to_aa (78 -> 75), tgm_rotmat_to_aa and its backward (finite at R == I,
    against the value continued from 1e-4 rad), the bare Gram-Schmidt and Rodrigues pairs: every group of every entry point."""
    aa, group = re_.aa_table()
    s, _, _ = re_.sixd_table()
    n, n6 = len(aa), len(s)
    x75, x78 = re_.x75_rows(), re_.x78_rows()
    got78 = _call(lib.h_75_to_78, (n, 78), x75)
    got75 = _call(lib.h_78_to_75, (n6, 75), x78)
    assert np.array_equal(np.delete(got78, np.s_[3:9], 1), np.delete(f32(x75), np.s_[3:6], 1))
    assert np.array_equal(np.delete(got75, np.s_[3:6], 1), np.delete(f32(x78), np.s_[3:9], 1))
    R = re_.rotations().reshape(n, 9)
    bwd = _call(lib.h_rotmat_to_aa_bwd, (n, 9), R, re_.cotangent((n, 3), 23))
    assert np.isfinite(bwd).all()
    got = {"aa_to_sixd": got78[:, 3:9], "sixd_to_aa": got75[:, 3:6], "rotmat_to_aa": _call(lib.h_rotmat_to_aa, (n, 3), R),
           "rotmat_to_aa_bwd": bwd, "gs": _call(lib.h_gs_forward, (n6, 9), s),
           "gs_bwd": _call(lib.h_gs_backward, (n6, 6), s, re_.cotangent((n6, 3, 3), 24).reshape(n6, 9)),
           "rodrigues": _call(lib.h_rodrigues, (n, 9), aa),
           "rodrigues_bwd": _call(lib.h_rodrigues_bwd, (n, 3), aa, re_.cotangent((n, 3, 3), 25).reshape(n, 9))}
    bad = {name: re_.check_conversion(name, g, f"host {name}") for name, g in got.items()}
    assert not any(bad.values()), {k: v for k, v in bad.items() if v}


@pytest.mark.parametrize("output_type", ["aa", "matrot"])
@pytest.mark.parametrize("context", list(re_.vposer_joint_codes()))
def test_host_vposer_decode_inside_the_bars(lib, context, output_type):
    """sixd_to_rot_kernel's and vposer_out_bwd_kernel's bodies on the host (numpy's fp32 products stand in for the dense layers)."""
    case = re_.vposer_case(context, output_type, 5)
    if context == "branches":              # (the weights move every code a little: the joints must still sit in all four branches)
        counts = np.bincount(re_.quaternion_branch(case["R64"].reshape(-1, 3, 3)), minlength=4)
        assert counts.min() >= 4 * 5, counts
    hp = HostPipeline(synth.make_body_model(120, seed=0), case["vp"], np.zeros((0, 3), np.float32), [0])
    z, w = f32(case["z"]), f32(case["w"])
    h1, h2, O = hp.mlp_forward(z)
    codes = f32(O.reshape(-1, 6))
    n = codes.shape[0]
    rot = _call(lib.h_gs_forward, (n, 9), codes)
    if output_type == "aa":
        out = _call(lib.h_rotmat_to_aa, (n, 3), rot)
        dR = _call(lib.h_rotmat_to_aa_bwd, (n, 9), rot, w.reshape(n, 3))
    else:
        out, dR = rot, w.reshape(n, 9)
    dO = _call(lib.h_gs_backward, (n, 6), codes, dR).reshape(-1, 126)
    dz = hp.mlp_backward(dO, h1, h2)
    assert not re_.check_vposer(case, out, dz, f"host vposer {context} {output_type}")


@pytest.mark.parametrize("name", ["rest", "tiny", "near_half", "exact_half", "pi_x"])
def test_host_pose_chain_inside_the_bars(lib, name):
    """pose_forward / pose_backward with axis-angle joints (the operator's path) at the edge poses: the 55 joints and the gradients of
    a joints-only loss, per frame."""
    case = re_.body_case(name, use_verts=False)
    hp = HostPipeline(case["bm"], synth.make_vposer(seed=1), np.zeros((0, 3), np.float32), [0])
    inp = case["inputs"]
    B = case["wj"].shape[0]
    z = lambda k, w: np.zeros((B, w)) if inp[k] is None else inp[k]
    X = np.zeros((B, 78), np.float32)
    X[:, 0:3], X[:, 9:19], X[:, 51:63], X[:, 63:75] = inp["transl"], inp["betas"], z("left_hand_pose", 12), z("right_hand_pose", 12)
    AA = f32(np.concatenate([z("global_orient", 3), z("body_pose", 63)], 1))
    Rm, PF, Jr = np.zeros((B, 495), np.float32), np.zeros((B, 486), np.float32), np.zeros((B, 165), np.float32)
    G, A = np.zeros((B, 660), np.float32), np.zeros((B, 660), np.float32)
    lib.h_pose_forward_aa(hp.h, B, P(X), P(AA), P(Rm), P(PF), P(Jr), P(G), P(A))
    joints = G.reshape(B, 55, 12)[:, :, [3, 7, 11]] + X[:, None, 0:3]
    dX, dAA = np.zeros((B, 78), np.float32), np.zeros((B, 66), np.float32)
    lib.h_pose_backward_aa(hp.h, B, P(X), P(AA), P(Rm), P(Jr), P(G), None, None, None, None, P(f32(case["wj"].reshape(B, 165))), P(dX), P(dAA))
    grads = {"global_orient": dAA[:, 0:3], "body_pose": dAA[:, 3:66], "betas": dX[:, 9:19], "left_hand_pose": dX[:, 51:63],
             "right_hand_pose": dX[:, 63:75], "transl": dX[:, 0:3]}
    assert all(np.isfinite(g).all() for g in grads.values())
    assert not re_.check_body(case, None, joints, grads, f"host pose chain {name}")
