// Op 1's whole backward (fdcap_chamfer_bwd_both): the gradient of both distance halves with respect to both point sets, in a
// DEFINED order -- no float atomics, so the result is the same bits in every run, whatever the launch geometry.
//
// A point's gradient is its own term minus the terms of everything that chose it as nearest neighbour:
//     a[b,i] = (2 g1[b,i]) (x1[b,i] - x2[b,idx1[b,i]])        u[b,j] = (2 g2[b,j]) (x2[b,j] - x1[b,idx2[b,j]])
//     gxyz1[b,i] = a[b,i] - S1,  S1 = +0 + u[b,j] over idx2[b,j] == i, ascending j
//     gxyz2[b,j] = u[b,j] - S2,  S2 = +0 + a[b,i] over idx1[b,i] == j, ascending i
//     reduce2:   gxyz2[j] = U - A,  U = +0 + u[b,j] ascending b,  A = +0 + a[b,i] over idx1[b,i] == j, ascending (b, i)
// every operation fp32 and rounded on its own (contraction is off in the kernel: no product is fused into an add); a missing
// term is +0; an index outside its range (-1: "no neighbour") makes its term +0 and is never used as an address.
//
// How: the contributions of one side, which sit in (b, i) order, are GROUPED BY DESTINATION with the stable LSD radix sort the
// repository already has (per-tile histogram sc_rs_hist_kernel, row prefixes nn_qs_rows_kernel, scatter nn_qs_scatter_kernel:
// fdc_scene.h), on the key b * dests + idx (idx alone for reduce2; out-of-range indices get the key one past the last
// destination), 8 bits per pass, as many passes as the largest key needs.  Stable: inside a destination's run the positions stay
// ascending.  Then one lane per DESTINATION finds its run by binary search in the sorted keys and adds it up in order, forming
// each term from the points as it goes (no term is stored).  Launches: 1 + 3 per pass + 1 per output, independent of B.
#pragma once
#include <hip/hip_runtime.h>

#include "fdc_scene.h"

namespace fdc {

static_assert(SC_RS_TILE == QS_TILE, "the histogram and the scatter kernel cut the keys into the same tiles");

// contributions a call can group: the tiles' last round must stay inside int
constexpr long long CB_MAX_SORT = 0x7fffffffLL - 2 * QS_TILE;

static inline int cb_blocks(long long n) { return (int)((n + QS_TILE - 1) / QS_TILE); }
static inline int cb_passes(unsigned maxkey) { int p = 1; while (p < 4 && (maxkey >> (8 * p)) != 0u) ++p; return p; }
// unsigned words of sort scratch for n contributions: keys [2][n] | histogram [256 x tiles] | digit totals [256]
static inline size_t cb_key_words(long long n) { return 2 * (size_t)n + 256 * (size_t)cb_blocks(n) + 256; }

// key[p] = destination of contribution p = (b, i): b * ndest + idx[p] (per_batch) or idx[p]; `invalid` for an index outside [0, ndest)
__global__ __launch_bounds__(256) void cb_keys_kernel(const int* __restrict__ idx, int total, int cnt, int ndest, int per_batch,
                                                      unsigned invalid, unsigned* __restrict__ key, int* __restrict__ val) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const int j = idx[p];
    const unsigned b = (unsigned)(p / cnt);
    key[p] = (j >= 0 && j < ndest) ? (per_batch ? b * (unsigned)ndest + (unsigned)j : (unsigned)j) : invalid;
    val[p] = (int)p;
}

// Groups the `total` = B * cnt contributions by destination.  key / val: [2][total]; hist: [256 x tiles + 256].  *buf: which half
// of key / val holds the sorted result.
static inline hipError_t cb_group(const int* idx, int B, int cnt, int ndest, bool per_batch, unsigned* key, int* val, unsigned* hist,
                                  hipStream_t st, int* buf) {
    const int total = B * cnt, nb = cb_blocks(total);
    const unsigned invalid = per_batch ? (unsigned)B * (unsigned)ndest : (unsigned)ndest;
    unsigned* const tot = hist + 256 * (size_t)nb;
    hipLaunchKernelGGL(cb_keys_kernel, dim3((total + 255) / 256), dim3(256), 0, st, idx, total, cnt, ndest, per_batch ? 1 : 0, invalid, key, val);
    const int passes = cb_passes(invalid);
    for (int pass = 0; pass < passes; ++pass) {
        const size_t a = (size_t)(pass & 1) * total, b = (size_t)((pass & 1) ^ 1) * total;
        hipLaunchKernelGGL(sc_rs_hist_kernel, dim3(nb), dim3(256), 0, st, key + a, total, 8 * pass, hist, nb);
        hipLaunchKernelGGL(nn_qs_rows_kernel, dim3(64), dim3(256), 0, st, hist, nb, tot);
        hipLaunchKernelGGL((nn_qs_scatter_kernel<QS_ROUNDS>), dim3(nb), dim3(256), 0, st, key + a, val + a, key + b, val + b, total, 8 * pass, hist, tot, nb);
    }
    *buf = passes & 1;
    return hipGetLastError();
}

// One side's gradient.  "Own" points xo [B][no] (batch stride so floats) are the destinations, "source" points xs [B][nsrc] (stride
// ss) the other set.  Own term of (b, d): (2 g_own[b,d]) (xo[b,d] - xs[b,idx_own[b,d]]) (g_own == nullptr: +0).  Scattered term of
// source position p = (b, s): (2 g_src[p]) (xs[b,s] - xo[b,d]).  reduce == 0: out[b,d] = own - S.  reduce != 0 (so == 0):
// out[d] = U - A.
struct CbSide {
    const float* xo; long long so;
    const float* xs; long long ss;
    int B, no, nsrc;
    const float* g_own; const int* idx_own;
    const float* g_src;
    int reduce;
};
// Every operation of the two helpers rounds on its own: `contract(off)`, or a product and the add that takes it become one fma
// (the __f*_rn intrinsics do not help: they are inlined as plain operators that carry their own header's contraction setting).
// acc <- the own term of destination (b0, d); reduce: U, over all batches
__device__ __forceinline__ void cb_own_term(const CbSide& c, int b0, int d, float acc[3]) {
#pragma clang fp contract(off)
    acc[0] = acc[1] = acc[2] = 0.f;
    if (c.g_own == nullptr) return;
    const int b1 = c.reduce ? c.B : b0 + 1;
    for (int b = b0; b < b1; ++b) {
        const size_t p = (size_t)b * c.no + d;
        const int j = c.idx_own[p];
        if (j < 0 || j >= c.nsrc) continue;                    // (+0: U + 0 leaves U as it is)
        const float gg = 2.f * c.g_own[p];
        const float* const po = c.xo + (size_t)b * c.so + 3 * (size_t)d;
        const float* const ps = c.xs + (size_t)b * c.ss + 3 * (size_t)j;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = gg * (po[k] - ps[k]);
            acc[k] = c.reduce ? acc[k] + v : v;
        }
    }
}
// S <- S + the term source position p = (b, i) scatters to destination d
__device__ __forceinline__ void cb_add_term(const CbSide& c, int p, int d, float S[3]) {
#pragma clang fp contract(off)
    const int b = p / c.nsrc, i = p - b * c.nsrc;
    const float gg = 2.f * c.g_src[p];
    const float* const po = c.xo + (size_t)b * c.so + 3 * (size_t)d;
    const float* const ps = c.xs + (size_t)b * c.ss + 3 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float v = gg * (ps[k] - po[k]); S[k] = S[k] + v; }
}
__device__ __forceinline__ void cb_store(float* __restrict__ out, size_t t, const float acc[3], const float S[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * t + k] = acc[k] - S[k];
}

// Grouped form: skey / sval [nsorted] are the source positions grouped by destination key (cb_group; skey == nullptr: no scattered
// terms).  One lane per destination t = b * no + d (reduce: t = d), which is also its key.
__global__ __launch_bounds__(256) void cb_gather_kernel(CbSide c, const unsigned* __restrict__ skey, const int* __restrict__ sval, int nsorted,
                                                        float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long ndest = c.reduce ? (long long)c.no : (long long)c.B * c.no;
    if (t >= ndest) return;
    const int b0 = (int)((unsigned)t / (unsigned)c.no), d = (int)((unsigned)t - (unsigned)b0 * (unsigned)c.no);   // (t < 2^31)
    float acc[3], S[3] = {0.f, 0.f, 0.f};
    cb_own_term(c, b0, d, acc);
    if (skey != nullptr) {
        const unsigned want = (unsigned)t;
        int lo = 0, hi = nsorted;                              // first sorted position with key >= want
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (skey[mid] < want) lo = mid + 1; else hi = mid;
        }
        for (int s = lo; s < nsorted && skey[s] == want; ++s) cb_add_term(c, sval[s], d, S);
    }
    cb_store(out, (size_t)t, acc, S);
}

}  // namespace fdc
