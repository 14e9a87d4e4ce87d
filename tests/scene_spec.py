"""The scene tables of fdcap_set_scene and the MFMA filter's score, restated in numpy from the rules the comments of
csrc/fdc_scene.h and csrc/fdc_chamfer.h give -- an independent specification the device build is compared with byte for byte
(tests/test_gpu_scene_tables.py) and whose soundness is checked in fp64 (tests/test_scene_spec_cpu.py).  Nothing here calls into
the library, and nothing restates its code: the order is a numpy lexsort per k-d node, the bf16 rounding is spelled out on the bits.

Float32 arithmetic is numpy float32: one rounding per operation (no fused multiply-add), sqrt correctly rounded -- as fdc_scene.h
compiles its table arithmetic, with contraction off."""
import numpy as np

MF_CH = 512                     # points per cell (one work unit of the search)
TILE = 32                       # points per MFMA tile (a leaf of the k-d tree at most)
QUARTER = MF_CH // 4            # points per quarter cell
SUPER = 16                      # cells per super cell
K1, K2 = np.float32(1e-4), np.float32(8e-6)     # the filter's error bound eps = K1 X rc + K2 (X^2 + rc^2)

TABLES = ("scene", "sorted", "inv", "bounds", "qbounds", "sbounds", "frags", "centers")   # fdcap_debug_scene_hash's order

f32 = np.float32


# ---- bf16 ------------------------------------------------------------------------------------------------------------------------
def bf16_bits(a):
    """float32 -> bf16 bits, round to nearest, ties to even: keep the top 16 bits and add one when the dropped 16 bits are more
    than half an ulp, or exactly half with an odd kept part (a carry moves into the exponent: the next binade, or inf)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    keep, drop = u >> 16, u & 0xFFFF
    up = (drop > 0x8000) | ((drop == 0x8000) & ((keep & 1) == 1))
    return (keep + up.astype(np.uint32)).astype(np.uint16)


def bf16_value(h):
    return (np.asarray(h, dtype=np.uint32) << 16).view(np.float32)


# ---- the k-d cell order ------------------------------------------------------------------------------------------------------------
def order_spec(xyz, nodes=None):
    """Cell order of the points xyz [n, 3] float32 (fdc_scene.h, the specification at the top):
      * a node of m > 32 points is cut along the longest axis of its box -- extent fl(max - min) in float32, as both builds compare
        it; ties go to the lower axis;
      * the left part takes the first nleft = min(m - 1, (units // 2) * unit) points by (coordinate, original index), -0 == +0,
        with unit = 512 points while m > 512 and 32 points below, units = ceil(m / unit);
      * inside a leaf (<= 32 points: one MFMA tile) the points stay in input order.
    Returns order [n] int64 (position -> original index).  `nodes`, if a list, receives (start, size, axis, nleft) of every cut."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    key = xyz + f32(0.0)                                    # -0 + 0 = +0: signed zeros compare equal
    n = xyz.shape[0]
    order = np.arange(n, dtype=np.int64)
    stack = [(0, n)] if n else []
    while stack:
        a, b = stack.pop()
        m = b - a
        seg = order[a:b]
        if m <= TILE:
            order[a:b] = np.sort(seg)
            continue
        unit = MF_CH if m > MF_CH else TILE
        nleft = min(m - 1, (-(-m // unit) // 2) * unit)
        p = xyz[seg]
        ext = p.max(0) - p.min(0)
        ax = int(np.argmax(ext))                            # first maximum: the lower axis on a tie
        order[a:b] = seg[np.lexsort((seg, key[seg, ax]))]   # by coordinate, then by original index
        if nodes is not None:
            nodes.append((a, m, ax, nleft))
        stack.append((a + nleft, b))
        stack.append((a, a + nleft))
    return order


# ---- the eight tables ----------------------------------------------------------------------------------------------------------------
def _pad(lo, hi):
    """fl(1e-6 + fl(1e-6 max(|lo|, |hi|))): the margin every box gets on both sides."""
    return f32(1e-6) + f32(1e-6) * np.maximum(np.abs(lo), np.abs(hi))


def _box(pts, valid):
    """min / max over the valid rows of pts [..., k, 3] (+inf / -inf where a group has none)"""
    lo = np.where(valid[..., None], pts, f32(np.inf)).min(-2)
    hi = np.where(valid[..., None], pts, f32(-np.inf)).max(-2)
    return lo, hi


def tables_spec(xyz, order):
    """All eight tables for the scene xyz [ns, 3] float32 in the cell order `order`, in their device layouts:
      scene   [ns, 4]  f32   input order  {x, y, z, bits(original index)}
      sorted  [ns, 4]  f32   cell order   {x, y, z, bits(original index)}
      inv     [ns]     i32   original index -> position
      bounds  [nchunk, 2, 4]      f32  cell box {lo, 0}, {hi, 0}, padded
      qbounds [nchunk, 4, 2, 4]   f32  quarter boxes, padded; a quarter without points: lo = hi = (+inf)^3
      sbounds [max(nsuper, 1), 2, 4] f32  boxes of 16 consecutive padded cell boxes, from lo = 1e30, hi = -1e30
      frags   [nchunk, 16 tiles, 2 k-halves, 32 points, 4] u32  bf16 MFMA fragments (below)
      centers [nchunk, 4]  f32   centre of the padded cell box, radius bound
    Fragment of a point, y' = fl(p - c) with c its cell's centre (padding rows: y' = 0, n2 = 1e30):
      h = bf16(y'), l = bf16(fl(y' - h)) per coordinate, then H = bf16(-2 h), L = bf16(-2 l) (exact);
      n2 = fl(z'^2 + fl(y'^2 + x'^2)) split in three: nh = bf16(n2), r = fl(n2 - nh), nm = bf16(r), nl = bf16(fl(r - nm));
      k-half 0 = [Hx Hx Lx Lx Hy Hy Ly Ly], k-half 1 = [Hz Hz Lz Lz nh nm nl 0] (bf16, low half of each word first).
    Radius bound: fl(fl(sqrt(max n2) * 1.00001) + 1e-6) over the cell's points."""
    with np.errstate(invalid="ignore", over="ignore"):       # (the padding of empty quarters: inf - inf, masked out)
        return _tables(np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3), np.asarray(order, dtype=np.int64))


def _tables(xyz, order):
    ns = xyz.shape[0]
    nchunk = -(-ns // MF_CH)
    nsuper = -(-nchunk // SUPER)
    npad = nchunk * MF_CH
    t = {}
    srt = np.zeros((ns, 4), np.float32)
    srt[:, :3] = xyz[order]
    srt[:, 3] = order.astype(np.int32).view(np.float32)
    t["sorted"] = srt
    sc = np.zeros((ns, 4), np.float32)
    sc[order] = srt
    t["scene"] = sc
    inv = np.zeros(ns, np.int32)
    inv[order] = np.arange(ns, dtype=np.int32)
    t["inv"] = inv

    P = np.zeros((npad, 3), np.float32)
    P[:ns] = srt[:, :3]
    valid = np.arange(npad) < ns

    lo, hi = _box(P.reshape(nchunk, MF_CH, 3), valid.reshape(nchunk, MF_CH))
    pad = _pad(lo, hi)
    blo, bhi = lo - pad, hi + pad
    b = np.zeros((nchunk, 2, 4), np.float32)
    b[:, 0, :3], b[:, 1, :3] = blo, bhi
    t["bounds"] = b

    qlo, qhi = _box(P.reshape(nchunk, 4, QUARTER, 3), valid.reshape(nchunk, 4, QUARTER))
    qpad = _pad(qlo, qhi)
    filled = (np.arange(nchunk)[:, None] * MF_CH + np.arange(4)[None, :] * QUARTER) < ns
    q = np.zeros((nchunk, 4, 2, 4), np.float32)
    q[:, :, 0, :3] = np.where(filled[..., None], qlo - qpad, f32(np.inf))
    q[:, :, 1, :3] = np.where(filled[..., None], qhi + qpad, f32(np.inf))
    t["qbounds"] = q

    s = np.zeros((max(nsuper, 1), 2, 4), np.float32)
    for su in range(nsuper):
        cells = b[su * SUPER:(su + 1) * SUPER]
        s[su, 0, :3] = np.minimum(f32(1e30), cells[:, 0, :3].min(0))
        s[su, 1, :3] = np.maximum(f32(-1e30), cells[:, 1, :3].max(0))
    t["sbounds"] = s

    cen = f32(0.5) * (blo + bhi)                                           # [nchunk, 3]
    yp = np.where(valid[:, None], P - np.repeat(cen, MF_CH, axis=0), f32(0.0))
    n2 = yp[:, 2] * yp[:, 2] + (yp[:, 1] * yp[:, 1] + yp[:, 0] * yp[:, 0])
    r2max = np.where(valid, n2, f32(0.0)).reshape(nchunk, MF_CH).max(1)
    n2 = np.where(valid, n2, f32(1e30))
    rad = np.sqrt(r2max) * f32(1.00001) + f32(1e-6)
    c = np.zeros((nchunk, 4), np.float32)
    c[:, :3], c[:, 3] = cen, rad
    t["centers"] = c

    h = bf16_bits(yp)
    l = bf16_bits(yp - bf16_value(h))
    H = bf16_bits(f32(-2.0) * bf16_value(h)).astype(np.uint32)
    L = bf16_bits(f32(-2.0) * bf16_value(l)).astype(np.uint32)
    nh = bf16_bits(n2)
    r1 = n2 - bf16_value(nh)
    nm = bf16_bits(r1)
    nl = bf16_bits(r1 - bf16_value(nm))
    nh, nm, nl = (v.astype(np.uint32) for v in (nh, nm, nl))
    f = np.zeros((nchunk, MF_CH // TILE, 2, TILE, 4), np.uint32)
    pair = lambda v: v | (v << 16)                                         # noqa: E731
    k0 = np.stack([pair(H[:, 0]), pair(L[:, 0]), pair(H[:, 1]), pair(L[:, 1])], 1)
    k1 = np.stack([pair(H[:, 2]), pair(L[:, 2]), nh | (nm << 16), nl], 1)
    f[:, :, 0] = k0.reshape(nchunk, MF_CH // TILE, TILE, 4)
    f[:, :, 1] = k1.reshape(nchunk, MF_CH // TILE, TILE, 4)
    t["frags"] = f
    return t


def scene_tables(xyz):
    return tables_spec(xyz, order_spec(xyz))


# ---- reading the fragments back ----------------------------------------------------------------------------------------------------
def frag_parts(frags, ch):
    """The cell's fragments as values [512, 3] of the -2-scaled hi and lo parts and [512, 3] of the three norm parts."""
    f = frags[ch].transpose(0, 2, 1, 3).reshape(MF_CH, 2, 4)   # [tile][k-half][point] -> [position in the cell][k-half]
    w0, w1 = f[:, 0], f[:, 1]
    lo16 = lambda w: (w & 0xFFFF).astype(np.uint16)        # noqa: E731
    H = np.stack([bf16_value(lo16(w0[:, 0])), bf16_value(lo16(w0[:, 2])), bf16_value(lo16(w1[:, 0]))], 1).astype(np.float64)
    L = np.stack([bf16_value(lo16(w0[:, 1])), bf16_value(lo16(w0[:, 3])), bf16_value(lo16(w1[:, 1]))], 1).astype(np.float64)
    N = np.stack([bf16_value(lo16(w1[:, 2])), bf16_value((w1[:, 2] >> 16).astype(np.uint16)), bf16_value(lo16(w1[:, 3]))],
                 1).astype(np.float64)
    return H, L, N


def _fma32(a, b, c):
    """fl(a b + c) for float32 operands: the product is exact in fp64, the sum is rounded to fp64 and then to fp32 (a double
    rounding that can move the result by one ulp in rare ties -- immaterial to the bound this feeds)."""
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)


def filter_error(tables, q, ch):
    """The MFMA filter's score of queries q (float32 [nq, 3]) against every point of cell ch, simulated from the cell's fragments
    and a query split the way nn_stream4_kernel splits it (fdc_chamfer.h): xx = fl(q - c), bf16 hi / lo parts, X2 = fma(z, z,
    fma(y, y, fl(x x))), X = fl(sqrt(X2) 1.000001); every bf16 x bf16 product is exact and the sum is taken in fp64.
    Returns (|score + X2 - d| [nq, k], eps [nq]) over the cell's k valid points, d the fp64 squared distance of the fp32 query and
    point, eps = K1 X rc + K2 (X2 + rc^2) the bound the filter assumes (|score + X2 - d| <= eps / 1.5)."""
    ns = tables["sorted"].shape[0]
    c = tables["centers"][ch]
    rc = c[3]
    q = np.asarray(q, dtype=np.float32).reshape(-1, 3)
    xx = q - c[None, :3]
    X2 = _fma32(xx[:, 2], xx[:, 2], _fma32(xx[:, 1], xx[:, 1], xx[:, 0] * xx[:, 0]))
    X = np.sqrt(X2) * f32(1.000001)
    qh = bf16_bits(xx)
    ql = bf16_bits(xx - bf16_value(qh))
    qh, ql = bf16_value(qh).astype(np.float64), bf16_value(ql).astype(np.float64)   # [nq, 3]
    H, L, N = frag_parts(tables["frags"], ch)
    k = min(MF_CH, ns - ch * MF_CH)
    H, L = H[:k].T, L[:k].T
    score = (qh @ H + ql @ H) + (qh @ L + ql @ L) + N[:k].sum(1)[None, :]           # [nq, k]: the 4 x 3 + 3 products of K = 16
    p = tables["sorted"][ch * MF_CH:ch * MF_CH + k, :3].astype(np.float64)
    d = ((q.astype(np.float64)[:, None, :] - p[None, :, :]) ** 2).sum(2)
    eps = K1 * X * rc + K2 * (X2 + rc * rc)
    return np.abs(score + X2.astype(np.float64)[:, None] - d), eps.astype(np.float64)


# ---- the edge scenes both test files run -----------------------------------------------------------------------------------------
EDGE_SIZES = (1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 639, 8191, 8192, 8193, 8321, 16385)


def edge_scenes():
    """(name, xyz float32 [n, 3]) of the scenes where the tables have edges: every count of filled quarters in the last cell
    (ns % 512) and ragged super cells, extent-0 boxes, flat axes, ties, signed zeros, scenes far from the origin."""
    from fdcap_amd import synth
    from tests.test_gpu_setup import _scenes
    for ns in EDGE_SIZES:
        rng = np.random.default_rng(ns)
        yield f"n{ns}", rng.uniform(-3, 3, (ns, 3)).astype(np.float32)
    yield "identical", np.tile(np.float32([[0.25, -1.5, 2.0]]), (700, 1))          # every box: extent 0, the pad alone
    yield "identical_far", np.tile(np.float32([[-3e4 + 0.5, 1e3, 7.0]]), (600, 1))
    rng = np.random.default_rng(5)
    line = np.zeros((3000, 3), np.float32)
    line[:, 0] = rng.uniform(-2, 2, 3000)
    line[:, 1], line[:, 2] = 0.3, -0.7                                                  # two flat axes
    yield "line", line
    for name, xyz in _scenes():
        yield f"setup_{name}", xyz
    yield "room_plus1e3", synth.make_scene(30000, seed=21) + np.float32(1e3)
    # a floor and a wall on a 1 mm grid, 30 km out on x (where the float32 spacing is 2 mm: ties along x everywhere)
    i, j = np.meshgrid(np.arange(140), np.arange(140), indexing="ij")
    floor = np.stack([i.ravel() * 1e-3, j.ravel() * 1e-3, np.zeros(i.size)], 1)
    i, k = np.meshgrid(np.arange(140), np.arange(60), indexing="ij")
    wall = np.stack([np.full(i.size, 0.14), i.ravel() * 1e-3, k.ravel() * 1e-3], 1)
    mm = np.concatenate([floor, wall]) + [-3e4, 0.0, 0.0]
    yield "mm_minus3e4", mm[np.random.default_rng(6).permutation(len(mm))].astype(np.float32)
    yield "room100k", synth.make_scene(100_000, seed=7)
