"""The rotation conversions of csrc/fdc_math.h at the inputs where they are piecewise or singular: one table of named cases, the
oracle's values in both precisions, the bars, and mutants (no GPU needed).

gs_forward / gs_backward, rodrigues_forward / rodrigues_backward, tgm_aa_to_rotmat, tgm_rotmat_to_aa and tgm_rotmat_to_aa_backward have
a Taylor branch (th2 <= 1e-6), four quaternion branches with a sign rule and a select at s2 == 0, a + 1e-8 offset under a division, and
clamps at 1e-12.  The older tests draw generic angles (0.01 .. 3.1 rad on the host build, |aa| ~ 1.7 on the device); the product meets
the rest pose (every argument of ops.BodyModel left None, the inner fit's jaw), half turns (SMPLify-X results in a camera frame,
fdcap_fit2d_flip_orient), and 6D codes that an optimiser has scaled and sheared.

CASES.  aa_table(): axis-angle rows, rounded to fp32 and held in fp64, each with a group label:
  rest                     exact zeros
  tiny:<theta>             3 random axes x theta in TINY, which straddles th2 = 1e-6 (theta = 1e-3)
  near_half:<delta>        3 random axes x (pi - delta), delta in 1e-1, 1e-2, 1e-3
  exact_half:<delta>       3 random axes x (pi - delta), delta in 1e-5, 0; exact_half:axes = +-pi about x, y, z
  quarter                  pi / 2 about x, y, z
  branches:<k>             10 random rotations in each quaternion branch k of tgm_rotmat_to_aa.  k = 0, 1, 2 from theta in
                           [2.2, 3.1]; branch 3 needs r22 >= 1e-6 and r00 + r11 >= 0, i.e. a trace above 1e-6, and the trace is
                           1 + 2 cos(theta) < 0 from 2 pi / 3 on, so no rotation of [2.2, 3.1] is in it: its rows are drawn from
                           theta in [1.2, 2.0]
  generic                  16 randn rows (|aa| ~ 1.7: what the older tests pin)
sixd_table(): 6D codes (the decoder's interleaved layout) of these rotations -- exact:<group> the first two columns of every row's
rotation; for the rows of generic, near_half, exact_half: scaled:<group> (first column x 0.2, second x 3), sheared:<group>
(cos(a1, a2) = 0.9), parallel:<group> (cos(a1, a2) = 0.9998); identity = (1, 0, 0, 1, 0, 0) exactly.

BARS.  Every entry point's oracle (oracle/rotrepr.py, oracle/tgm.py, oracle/smplx.py, oracle/vposer.py) is evaluated in fp64 and in
fp32 at the same fp32-rounded inputs, and
    bar = M max( max|o32 - o64| , 2^-24 max|o64| )          M, EPS32 of tests/gradient_bars.py; absolute, no rtol
is cut per group label for the conversions (so per theta and per delta: tiny:0.0003's Rodrigues gradient, whose fp32 oracle loses
1 - cos to cancellation, and the nearly parallel codes keep their much larger spreads to themselves) and per joint / per frame for what
leaves VPoser and the body model.  Nothing here comes from the host harness or the kernels.

EXCUSED ROWS.  At a half turn theta axis and -theta axis are one rotation and one ulp of qw decides which of them R -> aa returns.  The
rows of EXCUSED_GROUPS (exact_half:*), and only those, are compared in rotation space: the fp64 Rodrigues of the returned vector against
the fp64 rotation under the bar formed the same way there, and |aa| <= pi + bar.  Every other row is compared vector against vector,
which is what shows a lost `qw < 0` rule.  tests/test_rotation_edges_cpu.py asserts that the two oracles agree directly on every other
row, so the number of excused rows is the table's.

R == I IN THE R -> aa BACKWARD.  The oracle's gradient is NaN there (torch.where over 0 / 0); the library differentiates the selected
branch k = 2 instead (csrc/fdc_math.h).  Expected: the mean of the fp64 oracle's gradients at rotations of 1e-4 rad about x, y and z (it is
continuous at I); bar: the rule above over those three evaluations plus the largest difference among them.

MUTANTS: torch variants of the oracle's functions, each a defect a kernel could have; each must leave the bars by a factor of at least
2 in some group (tests/test_rotation_edges_cpu.py), so that the tests which use these bars cannot pass vacuously."""
import dataclasses
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import rotrepr, tgm
from oracle.smplx import batch_rodrigues
from oracle.vposer import VPoserDecoder
from tests.gradient_bars import EPS32, M

PI = float(np.pi)
TINY = (1e-7, 1e-5, 3e-4, 9.9e-4, 1.0e-3, 1.01e-3, 3e-3, 1e-2)
NEAR_HALF = (1e-1, 1e-2, 1e-3)
EXACT_HALF = (1e-5, 0.0)
EXCUSED_GROUPS = "exact_half"              # the group labels that hold it are compared in rotation space by R -> aa
PER_BRANCH = 10
DIRECT_AGREEMENT = 1e-4                    # |aa32 - aa64| of a non-excused row: far below the 2 pi of a sign flip
DT = {64: torch.float64, 32: torch.float32}


def f32(a):
    """rounded to fp32 (what the device is given), held in fp64"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _axes(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def rodrigues64(aa):
    """[n, 3] -> [n, 3, 3]: the exact exponential map in fp64 (sin x / x and (1 - cos x) / x^2 by series below 1e-4)"""
    aa = np.asarray(aa, dtype=np.float64).reshape(-1, 3)
    th = np.linalg.norm(aa, axis=1)
    small = th < 1e-4
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th * th / 6.0, np.sin(ths) / ths)
    b = np.where(small, 0.5 - th * th / 24.0, (1.0 - np.cos(ths)) / (ths * ths))
    K = np.zeros((aa.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -aa[:, 2], aa[:, 1], aa[:, 2], -aa[:, 0], -aa[:, 1], aa[:, 0]
    with np.errstate(invalid="ignore"):                         # (a mutant's NaN rows stay NaN)
        return np.eye(3) + a[:, None, None] * K + b[:, None, None] * (K @ K)


def quaternion_branch(R):
    """the branch (0 .. 3) tgm_rotmat_to_aa takes for rotations R [n, 3, 3] (the library looks at the transpose)"""
    R = np.asarray(R)
    rt = np.swapaxes(R, 1, 2)
    d2 = rt[:, 2, 2] < 1e-6
    return np.where(d2 & (rt[:, 0, 0] > rt[:, 1, 1]), 0, np.where(d2, 1, np.where(rt[:, 0, 0] < -rt[:, 1, 1], 2, 3)))


@functools.lru_cache(maxsize=None)
def aa_table():
    """-> aa [N, 3] (fp32 values in fp64), group [N] (labels)"""
    rng = np.random.default_rng(20)
    rows, group = [], []

    def add(name, a):
        a = f32(np.asarray(a, dtype=np.float64).reshape(-1, 3))
        rows.append(a)
        group.extend([name] * a.shape[0])

    add("rest", np.zeros((1, 3)))
    for th in TINY:
        add(f"tiny:{th:g}", _axes(rng, 3) * th)
    for d in NEAR_HALF:
        add(f"near_half:{d:g}", _axes(rng, 3) * (PI - d))
    for d in EXACT_HALF:
        add(f"exact_half:{d:g}", _axes(rng, 3) * (PI - d))
    add("exact_half:axes", np.concatenate([PI * np.eye(3), -PI * np.eye(3)]))
    add("quarter", 0.5 * PI * np.eye(3))
    for lo, hi, wanted in ((2.2, 3.1, (0, 1, 2)), (1.2, 2.0, (3,))):
        cand = f32(_axes(rng, 2000) * rng.uniform(lo, hi, (2000, 1)))
        br = quaternion_branch(f32(rodrigues64(cand)))
        for k in wanted:
            pick = np.nonzero(br == k)[0][:PER_BRANCH]
            assert len(pick) == PER_BRANCH, (k, len(pick))
            add(f"branches:{k}", cand[pick])
    add("generic", rng.standard_normal((16, 3)))
    return np.concatenate(rows), np.array(group)


def _code(a1, a2):
    """the decoder's layout: view(-1, 3, 2), a1 = (s0, s2, s4), a2 = (s1, s3, s5)"""
    return np.stack([a1, a2], axis=-1).reshape(-1, 6)


@functools.lru_cache(maxsize=None)
def sixd_table():
    """-> codes [N6, 6] (fp32 values in fp64), group [N6], source [N6] (the row of aa_table(), -1 for the identity code)"""
    aa, grp = aa_table()
    R = rodrigues64(aa)
    a1, a2 = R[:, :, 0], R[:, :, 1]
    sub = np.nonzero([g == "generic" or g.startswith(("near_half", "exact_half")) for g in grp])[0]
    codes, group, source = [_code(a1, a2)], ["exact:" + g for g in grp], [np.arange(len(grp))]
    for name, c1, c2 in (("scaled", 0.2 * a1[sub], 3.0 * a2[sub]),
                         ("sheared", a1[sub], 0.9 * a1[sub] + np.sqrt(1 - 0.9 ** 2) * a2[sub]),
                         ("parallel", a1[sub], 0.9998 * a1[sub] + np.sqrt(1 - 0.9998 ** 2) * a2[sub])):
        codes.append(_code(c1, c2))
        group += [name + ":" + g for g in grp[sub]]
        source.append(sub)
    codes.append(np.array([[1.0, 0, 0, 1, 0, 0]]))
    group.append("identity")
    source.append(np.array([-1]))
    return f32(np.concatenate(codes)), np.array(group), np.concatenate(source)


def excused(group):
    """[N] bool: the rows R -> aa is compared on in rotation space (a 6D code's label ends with its rotation's)"""
    return np.array([EXCUSED_GROUPS in g for g in group])


# ---- bars -------------------------------------------------------------------------------------------------------------------------------
def bar_of(o32, o64):
    o32, o64 = np.asarray(o32, dtype=np.float64), np.asarray(o64, dtype=np.float64)
    return M * max(float(np.abs(o32 - o64).max()), EPS32 * float(np.abs(o64).max()))


def group_bars(o32, o64, group):
    """{label: bar} over the rows (first axis) of each label"""
    return {g: bar_of(np.asarray(o32)[group == g], np.asarray(o64)[group == g]) for g in dict.fromkeys(group)}


def row_bars(o32, o64):
    """[n]: one bar per row (per joint, per frame)"""
    return np.array([bar_of(a, b) for a, b in zip(np.asarray(o32), np.asarray(o64))])


def _ratio(err, bar):
    """err / bar; a bar of 0 (an output that is exactly 0 in both precisions) must be matched exactly"""
    return err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))


def group_ratios(got, o64, bars, group):
    """{label: max|got - o64| / bar}; not finite anywhere in the group: inf"""
    got, o64, out = np.asarray(got, dtype=np.float64), np.asarray(o64, dtype=np.float64), {}
    for g, bar in bars.items():
        err = np.abs(got[group == g] - o64[group == g])
        out[g] = _ratio(float(err.max()), bar) if np.isfinite(err).all() else float("inf")
    return out


def row_ratios(got, o64, bars):
    got, o64 = np.asarray(got, dtype=np.float64), np.asarray(o64, dtype=np.float64)
    if len(bars) == 0:
        return np.zeros(0)
    err = np.abs(got - o64).reshape(len(bars), -1).max(1)
    return np.array([_ratio(e, b) if np.isfinite(e) else np.inf for e, b in zip(err, bars)])


def show(label, ratios):
    """prints max|err| / bar of every group (a dict) or row (an array) -> the worst"""
    items = list(ratios.items()) if isinstance(ratios, dict) else [(str(i), r) for i, r in enumerate(ratios)]
    worst = max((r for _, r in items), default=0.0)
    coarse = {}
    for g, r in items:
        k = g.split(":")[0] if not g.startswith(("exact:", "scaled:", "sheared:", "parallel:")) else ":".join(g.split(":")[:2])
        coarse[k] = max(coarse.get(k, 0.0), r)
    print(f"{label}: worst max|err| / bar {worst:.3g} |", " ".join(f"{k} {v:.3g}" for k, v in coarse.items()))
    return worst


def outside(ratios):
    items = ratios.items() if isinstance(ratios, dict) else enumerate(ratios)
    return {k: float(r) for k, r in items if not r <= 1.0}


def _t(a, p, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=DT[p], requires_grad=grad)


def _np(t):
    return t.detach().numpy().astype(np.float64)


# ---- the conversions' entry points: inputs and the oracle in both precisions ---------------------------------------------------------------
def x75_rows():
    """[N, 75] with the axis-angle table in columns 3:6, the rest random"""
    aa, _ = aa_table()
    x = f32(np.random.default_rng(21).standard_normal((aa.shape[0], 75)))
    x[:, 3:6] = aa
    return x


def x78_rows():
    """[N6, 78] with the 6D table in columns 3:9, the rest random"""
    s, _, _ = sixd_table()
    x = f32(np.random.default_rng(22).standard_normal((s.shape[0], 78)))
    x[:, 3:9] = s
    return x


def rotations():
    """the table's rotations as the device is given them: fp64 Rodrigues, rounded to fp32 -> [N, 3, 3]"""
    return f32(rodrigues64(aa_table()[0]))


def cotangent(shape, seed):
    return f32(np.random.default_rng(seed).standard_normal(shape))


def aa_to_sixd(p, fn=rotrepr.convert_to_6D_rot):
    """75 -> 78, columns 3:9"""
    with torch.no_grad():
        return _np(fn(_t(x75_rows(), p))[:, 3:9])


def sixd_to_aa(p, fn=rotrepr.convert_to_3D_rot):
    """78 -> 75, columns 3:6"""
    with torch.no_grad():
        return _np(fn(_t(x78_rows(), p))[:, 3:6])


def sixd_rotation64():
    with torch.no_grad():
        return _np(rotrepr.decode_6d(_t(sixd_table()[0], 64)))


def rotmat_to_aa(p, fn=rotrepr.matrot2aa):
    with torch.no_grad():
        return _np(fn(_t(rotations(), p)))


def rotmat_to_aa_bwd(p, R=None, g=None, fn=rotrepr.matrot2aa):
    """d (aa . g) / d R [n, 3, 3] at R (default: rotations(), g = cotangent(.., 23)); NaN where R == I"""
    R = rotations() if R is None else R
    g = cotangent((R.shape[0], 3), 23) if g is None else g
    Rt = _t(R, p, True)
    (fn(Rt) * _t(g, p)).sum().backward()
    return _np(Rt.grad)


def skew_rotations():
    """rotations of 1e-4 rad about x, y, z, rounded to fp32 -> [3, 3, 3]"""
    return f32(rodrigues64(1e-4 * np.eye(3)))


def rotmat_to_aa_bwd_at_identity(g, fn=rotrepr.matrot2aa):
    """g [n, 3] -> expected d / d R [n, 3, 3] at R == I and its bar [n] (module docstring)"""
    g = np.asarray(g, dtype=np.float64).reshape(-1, 3)
    R = skew_rotations()
    e = {p: np.stack([rotmat_to_aa_bwd(p, np.repeat(R[k:k + 1], len(g), 0), g, fn) for k in range(3)]) for p in (64, 32)}
    spread = np.abs(e[64][:, None] - e[64][None, :]).reshape(9, len(g), -1).max((0, 2))
    bars = np.array([bar_of(e[32][:, i], e[64][:, i]) for i in range(len(g))]) + spread
    return e[64].mean(0), bars


def gs(p, fn=rotrepr.decode_6d):
    with torch.no_grad():
        return _np(fn(_t(sixd_table()[0], p)))


def gs_bwd(p, fn=rotrepr.decode_6d):
    s = _t(sixd_table()[0], p, True)
    (fn(s) * _t(cotangent((s.shape[0], 3, 3), 24), p)).sum().backward()
    return _np(s.grad)


def rodrigues(p, fn=batch_rodrigues):
    with torch.no_grad():
        return _np(fn(_t(aa_table()[0], p)))


def rodrigues_bwd(p, fn=batch_rodrigues):
    r = _t(aa_table()[0], p, True)
    (fn(r) * _t(cotangent((r.shape[0], 3, 3), 25), p)).sum().backward()
    return _np(r.grad)


@functools.lru_cache(maxsize=None)
def conversions():
    """{entry point: {"o64", "o32", "group", "bar": {label: bar}}} for the seven device functions at the tables; for the two R -> aa
    forwards also "excused" [N] bool, "R64" (the rotation the returned vector must be) and "bar_R" (the excused rows' bars in rotation
    space, from the fp32 oracle's returned vector); for the R -> aa backward the rows with R == I hold the expected value of
    rotmat_to_aa_bwd_at_identity and "bar_row" [N] overrides the group's bar there."""
    _, ga = aa_table()
    _, gs6, _ = sixd_table()
    out = {}
    for name, fn, group in (("aa_to_sixd", aa_to_sixd, ga), ("sixd_to_aa", sixd_to_aa, gs6), ("rotmat_to_aa", rotmat_to_aa, ga),
                            ("rotmat_to_aa_bwd", rotmat_to_aa_bwd, ga), ("gs", gs, gs6), ("gs_bwd", gs_bwd, gs6),
                            ("rodrigues", rodrigues, ga), ("rodrigues_bwd", rodrigues_bwd, ga)):
        o64, o32 = fn(64), fn(32)
        e = {"o64": o64, "o32": o32, "group": group}
        if name in ("sixd_to_aa", "rotmat_to_aa"):
            e["excused"] = excused(group)
            e["R64"] = sixd_rotation64() if name == "sixd_to_aa" else rotations()
            e["bar_R"] = group_bars(rodrigues64(o32), e["R64"], group)
        if name == "rotmat_to_aa_bwd":
            at_i = np.nonzero(~np.isfinite(o64).all((1, 2)))[0]
            g = cotangent((len(group), 3), 23)
            want, bars = rotmat_to_aa_bwd_at_identity(g[at_i])
            o64, o32 = o64.copy(), o32.copy()
            o64[at_i], o32[at_i] = want, want
            e.update(o64=o64, o32=o32, at_identity=at_i, bar_row={int(i): float(b) for i, b in zip(at_i, bars)})
        e["bar"] = group_bars(e["o32"], e["o64"], group)
        if name == "rotmat_to_aa_bwd":
            for i in e["at_identity"]:
                e["bar"][group[i]] = e["bar_row"][int(i)]              # (a group of one row: `rest`)
        out[name] = e
    return out


def check_conversion(name, got, label=None):
    """`got` [N, ...] of entry point `name` against the fp64 oracle under the bars -> {label: max|err| / bar} of what is outside (the
    caller asserts that it is empty).  R -> aa: the excused rows in rotation space with |aa| <= pi + bar, the others directly."""
    e = conversions()[name]
    got = np.asarray(got, dtype=np.float64).reshape(e["o64"].shape)
    group = e["group"]
    if "excused" in e:
        ex = e["excused"]
        r = group_ratios(got[~ex], e["o64"][~ex], {g: b for g, b in e["bar"].items() if not excused([g])[0]}, group[~ex])
        rr = group_ratios(rodrigues64(got[ex]).reshape(-1, 3, 3), e["R64"][ex], {g: b for g, b in e["bar_R"].items() if excused([g])[0]}, group[ex])
        for g in rr:
            over = (np.linalg.norm(got[group == g], axis=1) - PI).max() / e["bar_R"][g]
            rr[g] = max(rr[g], float(over)) if np.isfinite(over) else float("inf")
        r.update(rr)
    else:
        r = group_ratios(got, e["o64"], e["bar"], group)
    show(label or name, r)
    return outside(r)


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------
def _m_taylor_wide(angle_axis):
    """aa -> R with the Taylor branch taken up to th2 <= 1e-4"""
    R = tgm.angle_axis_to_rotation_matrix(angle_axis)[:, :3, :3]
    rx, ry, rz = angle_axis[:, 0:1], angle_axis[:, 1:2], angle_axis[:, 2:3]
    k1 = torch.ones_like(rx)
    taylor = torch.cat([k1, -rz, ry, rz, k1, -rx, -ry, rx, k1], dim=1).view(-1, 3, 3)
    return torch.where(((angle_axis * angle_axis).sum(1) <= 1e-4).view(-1, 1, 1), taylor, R)


def _quaternion_trace_only(R):
    rt = R.transpose(1, 2)
    t3 = 1 + rt[:, 0, 0] + rt[:, 1, 1] + rt[:, 2, 2]
    q3 = torch.stack([t3, rt[:, 1, 2] - rt[:, 2, 1], rt[:, 2, 0] - rt[:, 0, 2], rt[:, 0, 1] - rt[:, 1, 0]], -1)
    return q3 / torch.sqrt(t3.view(-1, 1)) * 0.5


def _m_trace_only(R):
    """R -> aa always through the trace (fourth) candidate"""
    return tgm.quaternion_to_angle_axis(_quaternion_trace_only(R.reshape(-1, 3, 3)))


def _m_no_qw_rule(R):
    """R -> aa without the qw < 0 sign rule"""
    q = tgm.rotation_matrix_to_quaternion(F.pad(R.reshape(-1, 3, 3), [0, 1]))
    s2 = (q[:, 1:] ** 2).sum(1)
    s = torch.sqrt(s2)
    k = torch.where(s2 > 0.0, 2.0 * torch.atan2(s, q[:, 0]) / s, 2.0 * torch.ones_like(s))
    return q[:, 1:] * k[:, None]


def _m_rodrigues_no_offset(r):
    angle = torch.norm(r, dim=1, keepdim=True)
    return _rodrigues_from(r, angle)


def _m_rodrigues_no_dth(r):
    """the value of batch_rodrigues, its gradient without the path through th = |r + 1e-8|"""
    return _rodrigues_from(r, torch.norm(r + 1e-8, dim=1, keepdim=True).detach())


def _rodrigues_from(r, angle):
    n = r.shape[0]
    rot_dir = r / angle
    cos, sin = torch.cos(angle).unsqueeze(1), torch.sin(angle).unsqueeze(1)
    rx, ry, rz = torch.split(rot_dir, 1, dim=1)
    zeros = torch.zeros((n, 1), dtype=r.dtype)
    K = torch.cat([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], dim=1).view(n, 3, 3)
    return torch.eye(3, dtype=r.dtype).unsqueeze(0) + sin * K + (1 - cos) * torch.bmm(K, K)


def _m_gs_no_ddu(s):
    """Gram-Schmidt whose backward lacks the -d du term into b1 (u = a2 - d b1 with b1 held)"""
    a = s.reshape(-1, 3, 2)
    b1 = F.normalize(a[:, :, 0], dim=1)
    dot = torch.sum(b1 * a[:, :, 1], dim=1, keepdim=True)
    b2 = F.normalize(a[:, :, 1] - dot * b1.detach(), dim=-1)
    return torch.stack([b1, b2, torch.cross(b1, b2, dim=1)], dim=-1)


def _conv75(mutant):
    def fn(x):
        return torch.cat([x[:, :3], mutant(x[:, 3:6])[:, :, :-1].reshape(-1, 6), x[:, 6:]], dim=-1)
    return fn


def _conv78(mutant):
    def fn(x):
        return torch.cat([x[:, :3], mutant(rotrepr.decode_6d(x[:, 3:9])), x[:, 9:]], dim=-1)
    return fn


def _bwd_zero_at_identity(p):
    """R -> aa backward returning zero at s2 == 0"""
    return np.nan_to_num(rotmat_to_aa_bwd(p), nan=0.0)


# name -> (entry point, precision the variant is evaluated in, evaluation).  trace_only is a defect of PRECISION (the candidates
# are one quaternion in exact arithmetic: near a half turn t3 = 1 + trace cancels to nothing), so it is evaluated as a kernel would
# compute it, in fp32; the others change the function and are evaluated in fp64.
MUTANTS = {
    "taylor_wide": ("aa_to_sixd", lambda: aa_to_sixd(64, _conv75(_m_taylor_wide))),
    "trace_only": ("sixd_to_aa", lambda: sixd_to_aa(32, _conv78(_m_trace_only))),
    "trace_only_R": ("rotmat_to_aa", lambda: rotmat_to_aa(32, _m_trace_only)),
    "no_qw_rule": ("sixd_to_aa", lambda: sixd_to_aa(64, _conv78(_m_no_qw_rule))),
    "no_qw_rule_R": ("rotmat_to_aa", lambda: rotmat_to_aa(64, _m_no_qw_rule)),
    "bwd_zero_at_identity": ("rotmat_to_aa_bwd", lambda: _bwd_zero_at_identity(64)),
    "rodrigues_no_offset": ("rodrigues", lambda: rodrigues(64, _m_rodrigues_no_offset)),
    "rodrigues_no_offset_bwd": ("rodrigues_bwd", lambda: rodrigues_bwd(64, _m_rodrigues_no_offset)),
    "rodrigues_no_dth": ("rodrigues_bwd", lambda: rodrigues_bwd(64, _m_rodrigues_no_dth)),
    "gs_no_ddu": ("gs_bwd", lambda: gs_bwd(64, _m_gs_no_ddu)),
}


def mutant_factor(name):
    """-> (the largest max|err| / bar over the groups, the group): how far the mutant leaves the bars of its entry point, compared
    exactly as the kernels are (check_conversion)"""
    entry, run = MUTANTS[name]
    out = check_conversion(entry, run(), label=f"mutant {name} ({entry})")
    if not out:
        return 0.0, None
    g = max(out, key=out.get)
    return out[g], g


# ---- VPoser with chosen codes -----------------------------------------------------------------------------------------------------------
def _rows(prefix, count, skip=0):
    _, g, _ = sixd_table()
    idx = [i for i, name in enumerate(g) if name.startswith(prefix)]
    assert len(idx) >= skip + count, (prefix, len(idx), skip, count)
    return idx[skip:skip + count]


def vposer_joint_codes():
    """{context: 21 rows of sixd_table()}: the 6D code each joint's output bias holds.
    edges     the exact codes of rest, one row of every tiny theta, one of every near_half delta, nine generic rows
    deformed  seven scaled, seven sheared, seven nearly parallel codes of generic and near_half rotations
    half      exact_half rotations: nine exact codes, four each scaled, sheared, nearly parallel ('aa' outputs excused)
    branches  five exact codes in each quaternion branch of R -> aa (its backward differentiates the branch taken), one quarter turn
    identity  joint 0 at the exact identity code with ZERO output weights (R == I on the device: s2 == 0), the rest generic"""
    ctx = {}
    ctx["edges"] = (_rows("exact:rest", 1) + [_rows(f"exact:tiny:{th:g}", 1)[0] for th in TINY]
                    + [_rows(f"exact:near_half:{d:g}", 1)[0] for d in NEAR_HALF] + _rows("exact:generic", 9))
    ctx["deformed"] = [i for k, s in (("scaled", 0), ("sheared", 3), ("parallel", 6))
                       for i in _rows(f"{k}:generic", 4) + _rows(f"{k}:near_half", 3, skip=s)]
    ctx["half"] = (_rows("exact:exact_half", 9) + _rows("scaled:exact_half", 4, 2) + _rows("sheared:exact_half", 4, 5)
                   + _rows("parallel:exact_half", 4, 8))
    ctx["branches"] = [i for k in range(4) for i in _rows(f"exact:branches:{k}", 5)] + _rows("exact:quarter", 1)
    ctx["identity"] = _rows("identity", 1) + _rows("exact:generic", 10, skip=6) + _rows("sheared:generic", 10, skip=4)
    assert all(len(v) == 21 for v in ctx.values())
    return ctx


def vposer_data(vp, context):
    """synth.make_vposer(...) -> the VPoserData of `context`: out_b = the 21 codes, out_w x 0.02 (so every joint sits at its code
    and the latent gradient still flows); `identity`: the six output rows of joint 0 are zero"""
    s, _, _ = sixd_table()
    out_w = (0.02 * np.asarray(vp.out_w, dtype=np.float64)).astype(np.float32)
    if context == "identity":
        out_w[0:6] = 0.0
    return dataclasses.replace(vp, out_b=s[vposer_joint_codes()[context]].reshape(126).astype(np.float32), out_w=out_w)


@functools.lru_cache(maxsize=None)
def _vposer_case(context, output_type, B, seed):
    from fdcap_amd import synth
    vp = vposer_data(synth.make_vposer(seed=seed), context)
    _, g6, _ = sixd_table()
    labels = g6[vposer_joint_codes()[context]]
    width = 3 if output_type == "aa" else 9
    rng = np.random.default_rng(100 + B)
    z, w = f32(rng.standard_normal((B, 32))), f32(rng.standard_normal((B, 21, width)))
    at_identity = context == "identity" and output_type == "aa"
    res = {}
    for p in (64, 32):
        data = vp
        if at_identity:                    # the oracle's 0 x NaN: joint 0 (zero weights) moved 1e-4 rad off I, where its gradient is finite
            b = np.array(vp.out_b)
            R = skew_rotations()[0]
            b[0:6] = _code(R[:, 0][None], R[:, 1][None])[0]
            data = dataclasses.replace(vp, out_b=b.astype(np.float32))
        zt = _t(z, p, True)
        out = VPoserDecoder.from_data(data, DT[p]).decode(zt, output_type=output_type).reshape(B, 21, width)
        (out * _t(w, p)).sum().backward()
        o = _np(out)
        if at_identity:
            o[:, 0] = 0.0                  # tgm_rotmat_to_aa(I) = 0 exactly
        res[p] = (o, _np(zt.grad))
    assert np.isfinite(res[64][1]).all() and np.isfinite(res[32][1]).all() and np.isfinite(res[64][0]).all() and np.isfinite(res[32][0]).all()
    o64, o32 = res[64][0].transpose(1, 0, 2), res[32][0].transpose(1, 0, 2)             # [21, B, width]
    ex = excused(labels) if output_type == "aa" else np.zeros(21, bool)
    with torch.no_grad():
        R64 = _np(VPoserDecoder.from_data(vp, DT[64]).decode(_t(z, 64), output_type="matrot")).reshape(B, 21, 3, 3).transpose(1, 0, 2, 3)
    bar = row_bars(o32, o64)
    if ex.any():
        bar_R = row_bars(rodrigues64(o32[ex].reshape(-1, 3)).reshape(ex.sum(), B, 9), R64[ex].reshape(ex.sum(), B, 9))
        bar[ex] = bar_R
    return dict(vp=vp, labels=labels, z=z, w=w, out64=o64, out32=o32, bar_out=bar, excused=ex, R64=R64, dz64=res[64][1], dz32=res[32][1],
                bar_dz=bar_of(res[32][1], res[64][1]))


def vposer_case(context, output_type, B, seed=1):
    """The decoder of `context` at B random latents and random output weights -> dict: "vp" (the VPoserData), "z" [B, 32], "w"
    [B, 21, 3 or 9], per joint "out64" / "out32" [21, B, .], "bar_out" [21] (rotation-space bars where "excused"), "R64" [21, B, 3, 3],
    "dz64" / "dz32" [B, 32] and "bar_dz"."""
    return _vposer_case(context, output_type, B, seed)


def check_vposer(case, out, dz, label):
    """the device's (or a mutant's) outputs [B, 21, .] and d z [B, 32] -> what is outside: {joint or "dz": ratio}"""
    B = case["z"].shape[0]
    got = np.asarray(out, dtype=np.float64).reshape(B, 21, -1).transpose(1, 0, 2)
    ex = case["excused"]
    r = np.zeros(21)
    r[~ex] = row_ratios(got[~ex], case["out64"][~ex], case["bar_out"][~ex])
    if ex.any():
        n = int(ex.sum())
        r[ex] = row_ratios(rodrigues64(got[ex].reshape(-1, 3)).reshape(n, B, 9), case["R64"][ex].reshape(n, B, 9), case["bar_out"][ex])
        over = (np.linalg.norm(got[ex], axis=2).max(1) - PI) / case["bar_out"][ex]
        r[ex] = np.maximum(r[ex], over)
    ratios = {f"{j}:{case['labels'][j]}": float(r[j]) for j in range(21)}
    err = np.abs(np.asarray(dz, dtype=np.float64) - case["dz64"])
    ratios["dz"] = float(err.max() / case["bar_dz"]) if np.isfinite(err).all() else float("inf")
    print(f"{label}: max|err| / bar outputs {max(r):.3g} (joint {int(np.argmax(r))}, {case['labels'][int(np.argmax(r))]}), d z {ratios['dz']:.3g}"
          f" (bar {case['bar_dz']:.3g}, max|g| {np.abs(case['dz64']).max():.3g})")
    return outside(ratios)


# ---- the body model at edge poses -------------------------------------------------------------------------------------------------------
def body_poses():
    """{case: {"global_orient" [B, 3] or None, "body_pose" [B, 63] or None, "jaw_pose" [B, 3] (some cases)}}, fp32 values.
    rest       every pose argument None (B = 3)
    tiny       frame i: theta = TINY[i] for global_orient and all 21 body joints, each about its own random axis
    near_half  frame i: pi - NEAR_HALF[i] likewise
    exact_half frames pi - 1e-5 and pi about random axes, then global_orient = +-pi e_k with the body joints cycling through them
    pi_x       global_orient = (pi, 0, 0), a generic body pose (B = 3)
    jaw_*      a generic pose with jaw_pose = 0, tiny thetas, pi - 1e-3 and pi (the face operator; rest_jaw0: every other pose None)"""
    rng = np.random.default_rng(30)
    out = {"rest": {"B": 3, "global_orient": None, "body_pose": None}}

    def about_axes(thetas):
        th = np.asarray(thetas, dtype=np.float64)
        a = _axes(rng, len(th) * 22).reshape(len(th), 22, 3) * th[:, None, None]
        return {"B": len(th), "global_orient": f32(a[:, 0]), "body_pose": f32(a[:, 1:].reshape(len(th), 63))}

    out["tiny"] = about_axes(TINY)
    out["near_half"] = about_axes([PI - d for d in NEAR_HALF])
    half = about_axes([PI - d for d in EXACT_HALF])
    ax = np.concatenate([PI * np.eye(3), -PI * np.eye(3)])
    cyc = np.stack([np.roll(ax, -k, axis=0)[np.arange(21) % 6].reshape(63) for k in range(6)])
    out["exact_half"] = {"B": 8, "global_orient": f32(np.concatenate([half["global_orient"], ax])),
                         "body_pose": f32(np.concatenate([half["body_pose"], cyc]))}
    generic = lambda B: f32(rng.standard_normal((B, 63)) * 0.4)
    out["pi_x"] = {"B": 3, "global_orient": f32(np.tile([PI, 0, 0], (3, 1))), "body_pose": generic(3)}
    out["rest_jaw0"] = {"B": 2, "global_orient": None, "body_pose": None, "jaw_pose": np.zeros((2, 3))}
    out["jaw_zero"] = {"B": 2, "global_orient": f32(rng.standard_normal((2, 3)) * 0.8), "body_pose": generic(2), "jaw_pose": np.zeros((2, 3))}
    out["jaw_tiny"] = {"B": len(TINY), "global_orient": f32(rng.standard_normal((len(TINY), 3)) * 0.8), "body_pose": generic(len(TINY)),
                       "jaw_pose": f32(_axes(rng, len(TINY)) * np.asarray(TINY)[:, None])}
    out["jaw_half"] = {"B": 3, "global_orient": f32(rng.standard_normal((3, 3)) * 0.8), "body_pose": generic(3),
                       "jaw_pose": f32(_axes(rng, 3) * np.array([PI - 1e-3, PI - 1e-5, PI])[:, None])}
    return out


@functools.lru_cache(maxsize=None)
def body_case(name, V=120, seed=0, use_verts=True):
    """ops.BodyModel's oracle (tests/face_spec.py JawBody: oracle/smplx.py with the jaw's slot free) at the poses of body_poses()[name],
    random betas, hand coefficients and transl, loss = sum(wv . vertices) (if use_verts) + sum(wj . joints[:, :55]) -> dict: "inputs" (fp32 values;
    None: the argument is left out), "wv", "wj", per frame "verts64/32", "joints64/32", "bar_verts" [B], "bar_joints" [B], and per
    input "g64" / "g32" / "bar_g" ([B] per frame: the frames of a batch are independent)."""
    from fdcap_amd import synth
    from tests.face_spec import JawBody
    bm = synth.make_body_model(V, seed=seed)
    pose = body_poses()[name]
    B = pose["B"]
    rng = np.random.default_rng(40 + B)
    inp = {"global_orient": pose["global_orient"], "body_pose": pose["body_pose"], "betas": f32(rng.standard_normal((B, 10)) * 0.5),
           "left_hand_pose": None if name.startswith("rest") else f32(rng.standard_normal((B, 12)) * 0.3),
           "right_hand_pose": None if name.startswith("rest") else f32(rng.standard_normal((B, 12)) * 0.3),
           "transl": f32(rng.standard_normal((B, 3)))}
    if "jaw_pose" in pose:
        inp["jaw_pose"] = pose["jaw_pose"]
    widths = {"global_orient": 3, "body_pose": 63, "left_hand_pose": 12, "right_hand_pose": 12, "jaw_pose": 3}
    wv, wj = f32(rng.standard_normal((B, V, 3))), f32(rng.standard_normal((B, 55, 3)))
    res = {}
    for p in (64, 32):
        # an argument left None is zeros in the operator; the oracle is differentiated there all the same (the operator returns
        # no gradient for it, but the others' gradients pass through the same Rodrigues at 0)
        t = {k: _t(np.zeros((B, widths[k])) if v is None else v, p, True) for k, v in inp.items()}
        o = JawBody(bm, DT[p])(return_verts=True, **t)
        loss = (o.joints[:, :55] * _t(wj, p)).sum()
        if use_verts:
            loss = loss + (o.vertices * _t(wv, p)).sum()
        loss.backward()
        res[p] = (_np(o.vertices), _np(o.joints[:, :55]), {k: _np(v.grad) for k, v in t.items()})
    for p in (64, 32):
        assert all(np.isfinite(a).all() for a in (res[p][0], res[p][1], *res[p][2].values())), (name, p)
    return dict(bm=bm, inputs=inp, wv=wv, wj=wj, verts64=res[64][0], verts32=res[32][0], joints64=res[64][1], joints32=res[32][1],
                bar_verts=row_bars(res[32][0], res[64][0]), bar_joints=row_bars(res[32][1], res[64][1]), g64=res[64][2], g32=res[32][2],
                bar_g={k: row_bars(res[32][2][k], res[64][2][k]) for k in res[64][2]})


def check_body(case, verts, joints, grads, label):
    """the device's (or the host build's) vertices [B, V, 3], joints [B, 55, 3] (either may be None) and {input: gradient} -> what is
    outside: {"verts" / "joints" / input: the worst frame's max|err| / bar}"""
    r = {}
    if verts is not None:
        r["verts"] = float(row_ratios(verts, case["verts64"], case["bar_verts"]).max())
    if joints is not None:
        r["joints"] = float(row_ratios(joints, case["joints64"], case["bar_joints"]).max())
    for k, g in grads.items():
        r["d " + k] = float(row_ratios(g, case["g64"][k], case["bar_g"][k]).max())
    print(f"{label}: max|err| / bar", " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    return outside(r)


# ---- the optimiser's backward at a half-turn clip ------------------------------------------------------------------------------------------
HALF_TURN_CASE = (4, 120, 50, 1, 11)       # the smallest of gradient_bars.PARITY_CASES


class HalfTurnClip:
    """sc.term_gradients' / gradient_bars.start_state's `edit`: a clip as SMPLify-X leaves it in a camera frame -- every frame's
    global_orient replaced by (pi, 0, 0) composed with its own wobble (|aa| ~ pi: R -> aa off the trace branch, qw about 0), and
    the root 6D columns of frame 1 scaled (x 0.2, x 3) and of frame 3 sheared (cos = 0.9) before init(), as a few hundred Adam steps
    leave them (frame 2 is the case's outlier: init() overwrites it with frame 1, so it holds the scaled code as well)."""

    @staticmethod
    def clip(body_params):
        p = np.array(body_params, dtype=np.float64)
        R = rodrigues64(np.tile([PI, 0.0, 0.0], (p.shape[0], 1))) @ rodrigues64(p[:, 3:6])
        with torch.no_grad():
            p[:, 3:6] = _np(rotrepr.matrot2aa(torch.tensor(R)))
        return p.astype(np.float32)

    @staticmethod
    def rows(x78):
        x = x78.clone()
        a1, a2 = x[:, 3:9:2].clone(), x[:, 4:9:2].clone()
        x[1, 3:9:2], x[1, 4:9:2] = 0.2 * a1[1], 3.0 * a2[1]
        x[3, 4:9:2] = 0.9 * a1[3] + float(np.sqrt(1 - 0.9 ** 2)) * a2[3]
        return x


# ---- fdcap_fit2d_flip_orient ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flip_case():
    """global_orient rows for the flip (log(R(aa) R_y(pi)), Rodrigues then R -> aa): aa = 0 (the flip IS a half turn), pure yaw
    (0, theta, 0) up to theta = pi (the flip lands on R = I), (pi, 0, 0), (pi - 1e-3, 0, 0) and the exact_half rows -> dict: "aa",
    "group", "once64" (tests/fit2d_init_spec.py flip_rotation), "twice64" (the rotation itself), and the bars of both per group in
    rotation space, from the fp32 oracle's returned vectors."""
    from tests import fit2d_init_spec as fs
    aa, grp = aa_table()
    yaw = (1e-7, 1e-3, 0.5, 0.5 * PI, PI - 1e-3, PI)
    rows = [np.zeros((1, 3)), np.array([[0.0, th, 0.0] for th in yaw]), np.array([[PI, 0, 0], [PI - 1e-3, 0, 0]]), aa[excused(grp)]]
    group = np.array(["rest"] + [f"yaw:{th:.3g}" for th in yaw] + ["pi_x", "pi_x:0.001"] + list(grp[excused(grp)]))
    a = f32(np.concatenate(rows))
    flip = lambda r: rotrepr.matrot2aa(torch.matmul(batch_rodrigues(r), torch.diag(torch.tensor([-1.0, 1.0, -1.0], dtype=r.dtype))))
    with torch.no_grad():
        once32 = flip(_t(a, 32))
        twice32 = flip(once32)
    once64, twice64 = fs.flip_rotation(a), rodrigues64(a)
    return dict(aa=a, group=group, once64=once64, twice64=twice64, bar_once=group_bars(rodrigues64(_np(once32)), once64, group),
                bar_twice=group_bars(rodrigues64(_np(twice32)), twice64, group))
