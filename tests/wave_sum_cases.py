"""Inputs for the packed wave sums (csrc/fdc_math.h wave_sum64_pack), shared by the host test and the GPU test: [64][N] float32
per case, chosen so that any reassociation of wave_sum64's tree shows in the bits, and the tree itself in numpy as an independent
statement of it."""
import numpy as np

NS = (1, 3, 12, 16)
KINDS = ("spread", "huge", "cancel", "zeros", "naninf")


def case(kind, n, seed=0):
    rng = np.random.default_rng([seed, KINDS.index(kind), n])
    # magnitudes spread over 2^-20 .. 2^20, mixed signs: every partial sum rounds, so another association gives other bits
    v = (np.exp2(rng.uniform(-20, 20, (64, n))) * rng.choice([-1.0, 1.0], (64, n))).astype(np.float32)
    if kind == "huge":                                 # one huge lane per row (and per value): it swallows what is added before it
        for i in range(n):
            for row in range(4):
                v[16 * row + rng.integers(16), i] = np.float32(rng.choice([-1.0, 1.0]) * 2.0 ** rng.integers(40, 60))
    elif kind == "cancel":                             # a cancelling pair in one quad: the quad's sum keeps only its other two lanes
        for i in range(n):
            q = 4 * rng.integers(16)
            a, b = rng.choice(4, 2, replace=False)
            big = np.float32(2.0 ** 30 * (1 + rng.random()))
            v[q + a, i], v[q + b, i] = big, -big
    elif kind == "zeros":                              # zeros of both signs: all -0 sums to -0, one +0 among them to +0
        v[:] = np.where(rng.random((64, n)) < 0.5, np.float32(0.0), np.float32(-0.0))
        v[:, 0] = np.float32(-0.0)
        if n > 1:
            v[:, 1] = np.float32(-0.0)
            v[rng.integers(64), 1] = np.float32(0.0)
        if n > 2:
            v[rng.integers(64), 2] = np.float32(1.5)
    elif kind == "naninf":                             # a NaN lane and an Inf lane (one sign of infinity: no second NaN is born)
        for i in range(n):
            a, b = rng.choice(64, 2, replace=False)
            v[a, i] = np.float32(np.inf) if i % 2 == 0 else np.float32(-np.inf)
            if i % 3 != 2:
                v[b, i] = np.float32(np.nan)
    return np.ascontiguousarray(v)


def all_cases():
    return [(k, n, case(k, n)) for k in KINDS for n in NS]


def tree_sum(col):
    """wave_sum64's association on one value's 64 lanes, in float32: pairs, quads, octets, rows, then ((r0 + r1) + r2) + r3"""
    with np.errstate(all="ignore"):
        x = np.asarray(col, dtype=np.float32).reshape(4, 2, 2, 2, 2)
        pairs = x[..., 0] + x[..., 1]
        quads = pairs[..., 0] + pairs[..., 1]
        octets = quads[..., 0] + quads[..., 1]
        rows = octets[..., 0] + octets[..., 1]
        # (rows 2 and 3 pass through wave_sum64's masked steps before their own, which add +0.0: a row sum of -0.0 enters as +0.0)
        z = np.float32(0.0)
        return np.float32(np.float32(np.float32(rows[0] + rows[1]) + np.float32(rows[2] + z)) + np.float32(rows[3] + z))
