"""r22: the skinning backward forms its per-joint and per-frame sums in packed trees (csrc/fdc_math.h wave_sum64_pack: four values to a
quad, sixteen to a row).  Nothing computed may change by a bit.

1. The helper alone (fdcap_debug_wave_sum_pack, one wave): tests/wave_sum_cases.py's inputs -- what tests/test_wave_sum_pack_cpu.py runs
   on the host's lane model -- against wave_sum64 per value on the device, and against the tree as numpy states it.
2. The skinning backward through fdcap_opt_backward on 3 frames: dA, dtransl, dM, ds and dVoff as the launch left them
   (fdcap_debug_skin_bwd_sums) against the same state run through skin_bwd_small_kernel<., ., false>, which forms every sum by
   wave_sum64 on its own and stores from lane 0 as every earlier build did.  Contact sets of 4, 500 and 512 vertices with 4, 8 and 12
   skinning weights per vertex; the weights of the two larger sets are laid out so that one joint's list has exactly one entry, one
   has 65 (two trips of the lane loop) and one joint below the set's highest has none.  Two iterations of a clean clip -- the first
   search of a fit, then one that starts from its neighbours -- and the first iteration of a clip whose middle frame has a NaN
   translation.
"""
import ctypes

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.fitting import FittingOP, first_phase2_iter
from fdcap_amd.io import read_camerapose
from tests import wave_sum_cases as wsc

pytestmark = pytest.mark.gpu
NJ = 55


def _forms(reset):
    buf = ctypes.create_string_buffer(4096)
    capi.check(capi.load_library().fdcap_debug_kernel_forms(buf, len(buf), 1 if reset else 0), "kernel_forms")
    return buf.value.decode()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the helper alone

@pytest.mark.parametrize("n", wsc.NS)
@pytest.mark.parametrize("kind", wsc.KINDS)
def test_one_wave_of_the_packed_sums_gives_wave_sum64s_bits(kind, n):
    lib = capi.load_library()
    v = wsc.case(kind, n)
    packed, each = np.full(n, 7.0, np.float32), np.full(n, 9.0, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    capi.check(lib.fdcap_debug_wave_sum_pack(p(v), n, p(packed), p(each)), "fdcap_debug_wave_sum_pack")
    print(kind, n, [f"{w:08x}" for w in packed.view(np.uint32)], [f"{w:08x}" for w in each.view(np.uint32)])
    assert packed.tobytes() == each.tobytes()
    want = np.array([wsc.tree_sum(v[:, i]) for i in range(n)], dtype=np.float32)
    assert each.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the skinning backward

FRAMES, V, NS = 3, 700, 2000
J_ONE, J_65, J_NONE = 3, 6, 9                        # the joints with a list of one entry, of 65 entries, of none


def _weights(rng, vid, K, joints=21):
    """[len(vid), 55]: K non-zero weights per contact vertex on joints below `joints`, laid out for the three list lengths above"""
    nc = len(vid)
    w = np.zeros((nc, NJ), np.float32)
    free = [j for j in range(joints) if j not in (J_ONE, J_65, J_NONE)]
    for i in range(nc):
        js = rng.choice(free, K, replace=False)
        if nc >= 66:
            if i == 0: js[0] = J_ONE
            elif i <= 65: js[0] = J_65
        x = rng.random(K).astype(np.float32) + 0.05
        w[i, js] = x / x.sum()
    return w


@pytest.fixture(scope="module")
def skin_parts():
    return synth.make_vposer(seed=72), synth.make_scene(NS, seed=73)


@pytest.fixture
def streaming_search():
    lib = capi.load_library()
    capi.check(lib.fdcap_set_nn_kernel(2), "set_nn_kernel")            # the search form that leaves the neighbour records the vec kernel reads
    yield
    capi.check(lib.fdcap_set_nn_kernel(0), "set_nn_kernel")


def _x78(lib, params, n):
    x78 = torch.empty(n, 78, device="cuda")
    capi.check(lib.fdcap_params_75_to_78(capi.dptr(torch.tensor(params).cuda()), n, capi.dptr(x78), capi.current_stream()), "75->78")
    return x78


def _sums(fop, nc, reference):
    lib, h = fop.ctx.lib, fop.ctx.handle
    out = {"dA": torch.full((FRAMES, NJ * 12), 5.0, device="cuda"), "dtransl": torch.full((FRAMES, 3), 5.0, device="cuda"),
           "dM": torch.full((FRAMES, 12), 5.0, device="cuda"), "ds": torch.full((FRAMES,), 5.0, device="cuda"),
           "dVoff": torch.full((FRAMES, nc, 3), 5.0, device="cuda")}
    ja = ctypes.c_int32(-1)
    capi.check(lib.fdcap_debug_skin_bwd_sums(h, reference, *[capi.dptr(out[k]) for k in ("dA", "dtransl", "dM", "ds", "dVoff")],
                                             ctypes.byref(ja), capi.current_stream()), "fdcap_debug_skin_bwd_sums")
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["dA"] = out["dA"][:, :ja.value * 12]                           # (the rows the contact-set kernels write)
    return out, ja.value


@pytest.mark.parametrize("K", [4, 8, 12])
@pytest.mark.parametrize("nc", [4, 500, 512])
def test_skinning_backward_sums_against_one_sum_at_a_time(skin_parts, streaming_search, nc, K):
    vp, scene = skin_parts
    rng = np.random.default_rng([nc, K])
    bm = synth.make_body_model(V, seed=71, lbs_nnz=K)
    vid = np.sort(rng.choice(V, nc, replace=False))
    lbs = np.array(bm.lbs_weights, copy=True)
    lbs[vid] = _weights(rng, vid, K)
    bm.lbs_weights = lbs
    lists = (lbs[vid] != 0).sum(0)                                     # entries of every joint's list
    if nc >= 66: assert lists[J_ONE] == 1 and lists[J_65] == 65 and lists[J_NONE] == 0 and lists[J_NONE + 1:].any()
    else: assert (lists == 1).any() and (lists[:int(np.flatnonzero(lists).max())] == 0).any()
    clip = synth.make_clip(FRAMES, seed=74)
    P = first_phase2_iter(8)
    # a clean clip for two iterations, then one whose middle frame has a NaN translation (no neighbours: NaN sums, compared as bytes)
    # for the first iteration alone -- after a step the shared scale has made every frame NaN
    for nan_frame, iters in ((None, 2), (1, 1)):
        params = np.array(clip.body_params, copy=True)
        if nan_frame is not None: params[nan_frame, 0:3] = np.nan
        fop = FittingOP({"num_iter": 8}, {}, FRAMES, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid,
                        camera_ext=read_camerapose(clip.camerapose_lines), n_left=nc // 2)
        lib, h, st = fop.ctx.lib, fop.ctx.handle, capi.current_stream()
        fop.init(_x78(lib, params, FRAMES))
        _forms(True)
        good = [f for f in range(FRAMES) if f != nan_frame]
        for ii in range(iters):
            capi.check(lib.fdcap_opt_backward(h, ii, P, 0, st), "fdcap_opt_backward")
            got, ja = _sums(fop, nc, 0)
            want, _ = _sums(fop, nc, 1)
            assert ja > J_NONE or nc < 66
            for k in got:
                assert got[k].shape == want[k].shape and got[k].size
                diff = int((got[k].view(np.uint32) != want[k].view(np.uint32)).sum())
                print(f"nc {nc} K {K} NaN frame {nan_frame} iteration {ii} {k}: {diff} of {got[k].size} words differ")
                assert got[k].tobytes() == want[k].tobytes(), (nan_frame, ii, k, diff)
            if nan_frame is not None: assert np.isnan(got["dVoff"][nan_frame]).any() and np.isnan(got["dA"][nan_frame]).any()
            assert all(np.isfinite(got[k][good]).all() for k in got)
            assert np.abs(got["dA"][good]).max() > 0 and np.abs(got["dM"][good]).max() > 0
            if nc >= 66:                                               # the empty list's row is written, as zeros
                assert not got["dA"][good, 12 * J_NONE:12 * J_NONE + 12].any()
                assert got["dA"][0, 12 * J_ONE:12 * J_ONE + 12].any() and got["dA"][0, 12 * J_65:12 * J_65 + 12].any()
            capi.check(lib.fdcap_opt_step(h, ii, P, st), "fdcap_opt_step")
        forms = _forms(False)
        fop.close()
        assert "skin_bwd_vec_kernel" in forms, forms
