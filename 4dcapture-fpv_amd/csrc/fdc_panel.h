// Skinny-M fp32 GEMMs of the optimiser loop on v_mfma_f32_16x16x4_f32 (exact fp32: bitwise a k-ordered fmaf chain).
//
// Every dense contraction of an iteration multiplies a few hundred to a thousand frame rows by a STATIC matrix (VPoser
// weights, the contact set's pose/shape blend directions): M ~ 130..1028, N and K 32..1500.  At these sizes a classic
// LDS-tiled GEMM spends its time in per-launch latency (operand staging, barriers, split-K reductions), not on the matrix
// pipe.  Here the static operand is re-laid out ONCE, on the host, in MFMA fragment order ("panel"): the fragment of tile
// t / super-step s is 1 KiB that lane l reads as one float4 -- so a wave streams its B operand straight from L2 into
// registers with fully coalesced 16-byte loads, no LDS, no barrier; only the 16-row A block lives in LDS (k-blocked, so the
// A fragment of a super-step is one conflict-free ds_read_b128).  One super-step = 16 k = 4 MFMAs per (A read, B load).
//
//   panel_gemm_kernel          C[M,N] = A[M,K] x B            pose/shape blend offsets of the contact vertices (:280-283, K8)
//                                                             and their data gradient (B = the transposed panel)
//   vposer_fwd_fused_kernel    the three decoder layers (:270) in ONE launch: a workgroup owns 16 rows and one QUARTER of the
//                              hidden columns; layer 1 (K = 32) is recomputed by the four quarter-workgroups, layer 2 is
//                              split by output column, the output layer by K -- its four partial sums are added, in a fixed
//                              order, by the consumer (pose_fwd_kernel), so no workgroup ever waits for another
//   vposer_bwd_fused_kernel    the data-gradient chain dO -> dH2 -> dH1 -> d latent in one launch, split the other way round
//                              (every step is linear in its input once the LeakyReLU masks are applied, so K-slices of a
//                              step can run independently down to four partial latent gradients, summed by the Adam kernel)
// Against one LDS-tiled GEMM launch per product (six per iteration for the decoder, 55 us at 1028 rows): two launches of ~8 us each,
// and the two blend products' 25 + 24 us became ~12 + 12.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "fdc_forms.h"
#include "fdc_frame.h"
#include "fdc_loss.h"

namespace fdc {

// Lets the kernel(s) take `bytes` of dynamic LDS on the current device.  hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a property
// of ONE device's code object: `mask` (the launch site's own static) has one bit per device ordinal, set after the attribute took
// (two threads racing set it twice: harmless)
inline hipError_t fdc_allow_lds(std::atomic<uint64_t>& mask, size_t bytes, std::initializer_list<const void*> kernels) {
    int d = 0;
    (void)hipGetDevice(&d);
    const uint64_t bit = 1ull << (d & 63);
    if (mask.load() & bit) return hipSuccess;
    for (const void* k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    mask.fetch_or(bit);
    return hipSuccess;
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// B operand in fragment order: f[(tile * nss + s) * 64 + lane] = { B(16 s + 4 (lane >> 4) + m, 16 tile + (lane & 15)) }, m = 0..3
struct PanelB {
    const float4* f = nullptr;
    int ntile = 0;      // ceil(N / 16)
    int nss = 0;        // ceil(K / 16) super-steps
};

// host: B(k, n) = src[k * sk + n * sn], zero padded to whole tiles / super-steps
static inline void panel_pack(const float* src, long sk, long sn, int K, int N, std::vector<float>& out, int* ntile, int* nss) {
    const int nt = (N + 15) / 16, ns = (K + 15) / 16;
    out.assign((size_t)nt * ns * 256, 0.f);
    for (int t = 0; t < nt; ++t)
        for (int s = 0; s < ns; ++s)
            for (int l = 0; l < 64; ++l) {
                const int n = 16 * t + (l & 15);
                if (n >= N) continue;
                for (int m = 0; m < 4; ++m) {
                    const int k = 16 * s + 4 * (l >> 4) + m;
                    if (k < K) out[(((size_t)t * ns + s) * 64 + l) * 4 + m] = src[(long)k * sk + (long)n * sn];
                }
            }
    *ntile = nt;
    *nss = ns;
}

// device form of panel_pack (r6: a vertex set's panels are built where they are used -- the host loops cost 0.3 s per full-mesh set);
// one thread per fragment lane: out[(tile * nss + s) * 64 + lane]
__global__ __launch_bounds__(256) void panel_pack_kernel(const float* __restrict__ src, long sk, long sn, int K, int N, int nt, int ns,
                                                         float4* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)nt * ns * 64) return;
    const int l = (int)(idx & 63), s = (int)((idx >> 6) % ns), t = (int)((idx >> 6) / ns);
    const int n = 16 * t + (l & 15);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (n < N)
        for (int m = 0; m < 4; ++m) {
            const int k = 16 * s + 4 * (l >> 4) + m;
            if (k < K) v[m] = src[(long)k * sk + (long)n * sn];
        }
    out[idx] = make_float4(v[0], v[1], v[2], v[3]);
}

// LDS image of a 16-row A block, k-blocked: element (row i, column k) -- a super-step's fragment is lane-linear
__host__ __device__ __forceinline__ int pn_lds_index(int i, int k) { return (((k >> 2) << 4) + i) * 4 + (k & 3); }

// stage rows [r0, r0 + 16) x columns [k0, k0 + kn) of A (row-major, lda) as a k-blocked image of `kpad` columns
// (kpad % 16 == 0; rows >= rmax and columns >= kn are zero).  NT threads.
template <int NT>
__device__ __forceinline__ void panel_stage(float* __restrict__ sA, const float* __restrict__ A, int lda, int r0, int rmax,
                                            int k0, int kn, int kpad, int tid) {
    const bool vec = ((lda & 3) == 0) && ((k0 & 3) == 0) && ((((size_t)A) & 15) == 0);
    if (vec) {
        for (int e = tid; e < (kpad >> 2) * 16; e += NT) {          // e = kblock * 16 + row
            const int kb = e >> 4, i = e & 15, row = r0 + i, k = 4 * kb;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < rmax && k < kn) {
                const float* p = A + (size_t)row * lda + k0 + k;
                if (k + 3 < kn) v = *(const float4*)p;
                else { v.x = p[0]; if (k + 1 < kn) v.y = p[1]; if (k + 2 < kn) v.z = p[2]; }
            }
            *(float4*)(sA + (size_t)e * 4) = v;
        }
    } else {
        for (int e = tid; e < kpad * 16; e += NT) {                  // e = (kblock * 16 + row) * 4 + m
            const int kb = e >> 6, i = (e >> 2) & 15, k = 4 * kb + (e & 3), row = r0 + i;
            sA[e] = (row < rmax && k < kn) ? A[(size_t)row * lda + k0 + k] : 0.f;
        }
    }
}

// The fragment ring (PnRing, panel_prefetch, panel_mma below; PF fragments per tile in flight): loads in the main loop are
// unconditional and pinned by a scheduling barrier right after their issue.
// Loads under wave-uniform branches make hipcc wait vmcnt(0) in every super-step; unpinned, its scheduler sinks each load
// to just before its use -- either way one exposed L2 round trip per 4 MFMAs (the blend product ran 27 us instead of ~12).
// (Inline-asm loads with hand-counted s_waitcnt were tried and are wrong here: the ring is loop-carried, and the register
// copies hipcc inserts for it read a destination before the wait.)  The pins change no bits, only the schedule.
// (addresses are per-lane VGPR pairs: a scalar base would be written by SALU / v_readfirstlane right before the load reads
// it -- a 5-wait-state hazard hipcc does not pad inside an asm statement; measured: wrong fragments)
struct PnStream { const char* p; };                                   // this lane's byte address in a tile's fragment stream
__device__ __forceinline__ PnStream pn_stream(const float4* tile_base, int lane) { return PnStream{(const char*)(tile_base + lane)}; }
__device__ __forceinline__ f32x4_t pn_load_b(PnStream st, int step) { return *(const f32x4_t*)(st.p + (size_t)step * 1024); }
// nothing may be scheduled across this point: the fragment load issued before it stays PF super-steps ahead of its use
__device__ __forceinline__ void pn_pin() { __builtin_amdgcn_sched_barrier(0); }
__device__ __forceinline__ float4 pn_load_a(const float* __restrict__ p) { return *(const float4*)p; }
__device__ __forceinline__ f32x4_t pn_mfma(float a, float b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// The static fragment is the MFMA's A operand (its 16 rows = output columns n), the LDS block its B operand (its 16 columns =
// frame rows), so a lane's four results are FOUR CONSECUTIVE OUTPUT COLUMNS of one frame: lane (j = lane & 15, g = lane >> 4),
// register r  <->  out[frame j][16 tile + 4 g + r].  Epilogues are one 16-byte store per tile -- to global memory and into
// the next layer's k-blocked LDS image alike (the other way round each lane holds four frames of one column: four
// scattered 4-byte LDS writes with an 8-way bank conflict).
__device__ __forceinline__ f32x4_t pn_step(float4 a, f32x4_t b, f32x4_t acc) {
    acc = pn_mfma(b[0], a.x, acc);
    acc = pn_mfma(b[1], a.y, acc);
    acc = pn_mfma(b[2], a.z, acc);
    return pn_mfma(b[3], a.w, acc);
}
__device__ __forceinline__ float4 pn_f4(f32x4_t v) { return make_float4(v[0], v[1], v[2], v[3]); }

// Operand format of the exact-fp32 chain, as the one product loop (panel_mma) sees a format -- PnH2 below is the other one:
//   Frag / Stream   a static fragment's element type; a lane's handle on one tile's fragment stream
//   AFrag / BFrag   what a lane holds of one step: the LDS block's fragment, the static operand's
//   LdsElem / Lds   the LDS images' element type and their geometry (RB images `img` elements apart); the loop gets the first image at
//                   the first step as a __restrict__ pointer of its own
//   load_a          the LDS fragment of (row block, step, lane);   load_b   the static fragment of (stream, step)
//   Acc / step      one step's MFMAs on one accumulator
// One step = one super-step: 16 columns of K, four v_mfma_f32_16x16x4_f32.
struct PnF32 {
    typedef f32x4_t Acc;
    typedef float4 Frag;
    typedef float4 AFrag;
    typedef f32x4_t BFrag;
    typedef PnStream Stream;
    typedef float LdsElem;
    struct Lds { int img; };
    static __device__ __forceinline__ Stream stream(const Frag* tile_base, int lane) { return pn_stream(tile_base, lane); }
    static __device__ __forceinline__ AFrag load_a(const LdsElem* sA, const Lds& l, int rb, int step, int lane) {
        return pn_load_a(sA + (size_t)rb * l.img + (size_t)step * 256 + lane * 4);
    }
    static __device__ __forceinline__ BFrag load_b(Stream st, int step) { return pn_load_b(st, step); }
    static __device__ __forceinline__ Acc step(const AFrag& a, const BFrag& b, Acc acc) { return pn_step(a, b, acc); }
};

// Two register sets, each PF steps deep: set A is consumed while set B is being filled and vice versa, so no fragment
// register is redefined while its previous value is live and the ring needs no copies at the loop's back edge (with one
// set hipcc rotates the registers there and has to drain the queue once per turn).  The first set is loaded by
// panel_prefetch -- issued BEFORE the barrier / staging that precedes the product, so the first L2 round trip is hidden.
// F: the operand format (PnF32, PnH2); T tiles' streams share the LDS block(s).
template <class F, int T, int PF>
struct PnRing { typename F::BFrag bA[T][PF]; typename F::Stream st[T]; };

// bf[t]: tile t's fragments at the first step (without the lane offset)
template <class F, int T, int PF>
__device__ __forceinline__ void panel_prefetch(PnRing<F, T, PF>& rg, const typename F::Frag* const (&bf)[T], int nst, int lane) {
    const int last = nst - 1;
#pragma unroll
    for (int t = 0; t < T; ++t) rg.st[t] = F::stream(bf[t], lane);
#pragma unroll
    for (int p = 0; p < PF; ++p)
#pragma unroll
        for (int t = 0; t < T; ++t) rg.bA[t][p] = F::load_b(rg.st[t], min(p, last));
}

// Where inside a step of the main loop the two requests -- the NEXT step's LDS fragments, the static fragments PF steps ahead --
// and the pin stand.  The MFMAs and their order are the same in all three, so the order changes no bit; it does change hipcc's
// schedule and register count (NOTES, Round 10), and each is what its kernels were tuned with.  Whether one order serves all is
// an open tuning question.
enum class PnOrder {
    // static fragment -> pin -> next LDS fragments -> MFMAs.  The one-tile streams of the blend products: panel_gemm_kernel,
    // panel_gemm_wide_kernel, panel_gemm3_kernel, panel_gemm3_rb2_kernel, panel_gemm3_rb2k_kernel, panel_gemm3_wide_kernel,
    // blend_skin_fwd_kernel
    StaticPinLds,
    // next LDS fragment, then per tile: static fragment -> pin -> that tile's MFMAs.  The fused VPoser kernels' layers:
    // vposer_fwd_fused_kernel, vposer_bwd_fused_kernel, vposer_fwd_split3_kernel, vposer_bwd_split3_kernel
    LdsTilePin,
    // next LDS fragments -> all tiles' static fragments -> pin -> all MFMAs.  The K-split products: panel_gemm3_ksw_kernel,
    // panel_gemm3_kloop_kernel
    LdsStaticPin,
};

// acc[rb * T + t] += A_rb[16 x nst steps] * B_t: RB row blocks of 16 (LDS images) x T column tiles (fragment streams) per wave.  A
// step's RB LDS fragments are read ONCE for T tiles and its T static fragments once for RB row blocks.  lds: the images at the first
// step; rg: the ring panel_prefetch filled for the same nst (> 0).  The LDS fragments run one step ahead of their MFMAs.
// Main loop: 2 PF steps per turn, loads pinned.  Tail: at most 2 PF - 1 steps, step indices clamped to the last one, not pinned.
template <class F, int RB, int T, int PF, PnOrder ORD>
__device__ __forceinline__ void panel_mma(const typename F::LdsElem* __restrict__ sA, const typename F::Lds lds, PnRing<F, T, PF>& rg, int nst, typename F::Acc* acc, int lane) {
    typedef typename F::AFrag AF;
    typedef typename F::BFrag BF;
    BF (&bA)[T][PF] = rg.bA;
    BF bB[T][PF];
    const int last = nst - 1;
    AF a[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) a[rb] = F::load_a(sA, lds, rb, 0, lane);
    // one step on use[.][p]; it requests the LDS fragments of step `next` and fill[.][p] = the static fragments of step `fs`.
    // HEAD: the main loop's first half (pinned, both indices in range); BODY: its second half (pinned, indices clamped to the last step:
    // the loads stay unconditional); TAIL: clamped, not pinned; DRAIN: nothing left to request from the streams
    constexpr int HEAD = 0, BODY = 1, TAIL = 2, DRAIN = 3;
    auto step = [&](auto mode, BF (&use)[T][PF], BF (&fill)[T][PF], int p, int fs, int next) {
        constexpr int MODE = decltype(mode)::value;
        constexpr bool per_tile = ORD == PnOrder::LdsTilePin, pinned = MODE == HEAD || MODE == BODY;
        AF an[RB];
        auto load_an = [&]() {
            const int n = MODE == HEAD ? next : min(next, last);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) an[rb] = F::load_a(sA, lds, rb, n, lane);
        };
        auto load_fill = [&](int t) { fill[t][p] = F::load_b(rg.st[t], MODE == HEAD ? fs : min(fs, last)); };
        if (ORD != PnOrder::StaticPinLds) load_an();
        if (MODE != DRAIN && !per_tile) {
#pragma unroll
            for (int t = 0; t < T; ++t) load_fill(t);
            if (pinned) pn_pin();
        }
        if (ORD == PnOrder::StaticPinLds) load_an();
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (MODE != DRAIN && per_tile) {
                load_fill(t);
                if (pinned) pn_pin();
            }
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) acc[rb * T + t] = F::step(a[rb], use[t][p], acc[rb * T + t]);
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) a[rb] = an[rb];
    };
    const std::integral_constant<int, HEAD> head;
    const std::integral_constant<int, BODY> body;
    const std::integral_constant<int, TAIL> tail;
    const std::integral_constant<int, DRAIN> drain;
    int s = 0;
    for (; s + 2 * PF <= nst; s += 2 * PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) step(head, bA, bB, p, s + PF + p, s + p + 1);
#pragma unroll
        for (int p = 0; p < PF; ++p) step(body, bB, bA, p, s + 2 * PF + p, s + PF + p + 1);
    }
    // tail: fewer than 2 PF steps; set A holds the first PF of them
#pragma unroll
    for (int p = 0; p < PF; ++p)
        if (s + p < nst) step(tail, bA, bB, p, s + PF + p, s + p + 1);
#pragma unroll
    for (int p = 0; p < PF - 1; ++p)
        if (s + PF + p < nst) step(drain, bB, bA, p, 0, s + PF + p + 1);
}

#ifdef FDC_PN_TIMING
// instrumentation build only (never shipped): per-workgroup s_memtime stamps [block][8]
__device__ unsigned long long g_pn_times[8192 * 8];
#define PN_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x < 8192) g_pn_times[blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define PN_STAMP(i)
#endif

// workgroup -> (row block, column block), XCD-aware: PnMap / panel_map, fdc_forms.h.  blockIdx & 7 = XCD = (row group, column
// group), blockIdx >> 3 = slot inside the group.  on == false: a ragged group's surplus workgroup (the whole workgroup returns)
struct PnBlock { int rbk, cbk; bool on; };
__device__ __forceinline__ PnBlock panel_block(const PnMap& mp) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int r_in = mp.rfast ? slot % mp.rpg : slot / mp.cpg, c_in = mp.rfast ? slot / mp.rpg : slot % mp.cpg;
    const int rbk = (xcd / mp.xc) * mp.rpg + r_in, cbk = (xcd % mp.xc) * mp.cpg + c_in;
    return PnBlock{rbk, cbk, r_in < mp.rpg && c_in < mp.cpg && rbk < mp.nrb && cbk < mp.ncb};
}

// C[M, N] = A[M, K] x B.  Workgroup = 8 waves = 16 RB rows x 128 columns (a 16-column tile per wave); K in slabs of `kslab`
// columns (multiple of 16) so any K fits the LDS.  1-D grid of 8 * rpg * cpg workgroups (PnMap).
// Dynamic LDS: RB * kslab * 16 floats.
template <int RB>
__global__ __launch_bounds__(512) void panel_gemm_kernel(const float* __restrict__ A, int lda, int M, int K, PanelB B, int kslab,
                                                         float* __restrict__ C, int ldc, int N, PnMap mp) {
    extern __shared__ __attribute__((aligned(16))) float pn_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const PnBlock pb = panel_block(mp);
    if (!pb.on) return;
    const int rbk = pb.rbk, cbk = pb.cbk;
    const int tile = cbk * 8 + wave;
    const int m0 = rbk * (16 * RB);
    const int img = kslab * 16;
    PN_STAMP(0);
    f32x4_t acc[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[rb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const bool active = tile < B.ntile;
    const float4* const tf = B.f + (size_t)(active ? tile : 0) * B.nss * 64;
    for (int k0 = 0; k0 < K; k0 += kslab) {
        const int kn = min(kslab, K - k0), kpad = (kn + 15) & ~15;
        PnRing<PnF32, 1, 4> rg;
        const float4* bfp = tf + (size_t)(k0 >> 4) * 64;
        panel_prefetch<PnF32, 1, 4>(rg, {bfp}, kpad >> 4, lane);            // in flight while the A block is staged
        if (k0) __syncthreads();
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) panel_stage<512>(pn_lds + (size_t)rb * img, A, lda, m0 + 16 * rb, M, k0, kn, kpad, tid);
        __syncthreads();
        PN_STAMP(1);
        if (active) panel_mma<PnF32, RB, 1, 4, PnOrder::StaticPinLds>(pn_lds, {img}, rg, kpad >> 4, acc, lane);
    }
    PN_STAMP(2);
    const int n4 = tile * 16 + 4 * g;
    if (active && n4 < N) {
        const bool vec = ((ldc & 3) == 0) && ((((size_t)C) & 15) == 0) && n4 + 3 < N;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const int m = m0 + 16 * rb + j;
            if (m < M) {
                float* dst = C + (size_t)m * ldc + n4;
                if (vec) *(float4*)dst = pn_f4(acc[rb]);
                else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (n4 + r < N) dst[r] = acc[rb][r];
                }
            }
        }
    }
    PN_STAMP(3);
}

// ---------------------------------------------------------------------------------------------------------------------
// fp32 products on the 16-bit matrix cores: the operands are split into planes of 16-bit numbers (format PnH2 below) and a product
// becomes a few v_mfma_f32_16x16x32_f16 with fp32 accumulation -- 32 columns of K in a fraction of the cycles the fp32 form needs
// (eight v_mfma_f32_16x16x4_f32 = 256 cycles per SIMD), and the loop's products are bound by exactly that pipe (93 % of its issue
// slots).  tests/test_gpu_panel.py holds both forms to the same bar against fp64.
typedef float f32x4u_t __attribute__((ext_vector_type(4), aligned(4)));      // 16-byte store at 4-byte alignment (3 V is odd)
struct PanelB3 {
    const uint4* f = nullptr;       // f[((tile * nst + s) * 2 + plane) * 64 + lane] = 8 fp16: B(32 s + 8 (lane >> 4) + e, 16 tile + (lane & 15)), scaled
    int ntile = 0, nst = 0;         // ceil(N / 16), ceil(K / 32)
    const float* isc = nullptr;     // isc[16 tile + c] = 1 / (the power-of-two scale of output column c of the tile)
};

// ---------------------------------------------------------------------------------------------------------------------
// Operand format of the split products, PnH2 (late r5; three bf16 planes and six products per step until then): TWO fp16 planes and
// THREE products per step.
//   a s = h + 2^-11 l,  h = fp16(a s),  l = fp16((a s - h) 2^11)   (both conversions round to nearest even; a s - h is exact)
// with s a power of two per frame row of the dynamic operand (its largest |a| lands in [2^13, 2^14): found while the block is
// staged, one extra barrier) and per output column of the static one (host).  |a - (h + 2^-11 l) / s| <= 2^-22 |a| for every element
// within 2^-27 of its row's largest (below that: 2^-50 of the largest, absolutely).  Products h h -> one accumulator, l h + h l ->
// a second one, joined as (acc_h + 2^-11 acc_l) / (s_a s_b) in the epilogue (exact scalings, one rounding); l l (<= 2^-22 |a b|)
// is dropped.  Error <= 3 x 2^-22 |a||b| per term: far below the K 2^-24 bound of an fp32 fmaf chain, and
// tests/test_gpu_panel.py holds it to the same 1e-6 sum|a||b| bar against fp64.  Against the three-plane format: half the MFMA
// issue, two thirds of the fragment bytes and of the LDS reads per 32 columns of K -- all three of the resources these kernels sit
// on at once.
typedef _Float16 pn_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 pn_f16x2 __attribute__((ext_vector_type(2)));
typedef float pn_f32x2 __attribute__((ext_vector_type(2)));
static inline unsigned pn2_f16_host(float f) {                  // fp32 -> fp16 bits, round to nearest even (no libgcc soft-float call)
    unsigned u; memcpy(&u, &f, 4);
    const unsigned sign = (u >> 16) & 0x8000u, ex = (u >> 23) & 255u;
    unsigned man = u & 0x7FFFFFu;
    if (ex == 255u) return sign | 0x7C00u | (man ? 0x200u : 0u);
    const int e = (int)ex - 127 + 15;
    if (e >= 31) return sign | 0x7C00u;
    if (e <= 0) {                                               // subnormal or zero
        if (e < -10) return sign;
        man |= 0x800000u;
        const int sh = 14 - e;                                  // 14 .. 24
        const unsigned q = man >> sh, rem = man & ((1u << sh) - 1u), half = 1u << (sh - 1);
        return sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));
    }
    const unsigned q = ((unsigned)e << 10) | (man >> 13), rem = man & 0x1FFFu;
    return sign | (q + ((rem > 0x1000u || (rem == 0x1000u && (q & 1u))) ? 1u : 0u));   // a carry into the exponent is the right answer
}
static inline float pn2_f16f_host(unsigned h) {
    const unsigned sign = (h & 0x8000u) << 16, ex = (h >> 10) & 31u, man = h & 0x3FFu;
    float f;
    if (ex == 0) { f = ldexpf((float)man, -24); unsigned u; memcpy(&u, &f, 4); u |= sign; memcpy(&f, &u, 4); return f; }
    const unsigned u = sign | (ex == 31u ? 0x7F800000u : ((ex + 112u) << 23)) | (man << 13);
    memcpy(&f, &u, 4);
    return f;
}
__device__ __forceinline__ unsigned pn2_pk2(float a, float b) {
    const pn_f32x2 f = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f, pn_f16x2));
}
struct PnH2 {
    static constexpr int NP = 2, SC_U4 = 4 + 4 * 12;            // 16 inverse row scales + 16 partial maxima per wave (<= 12 waves)
    struct Acc { f32x4_t h, l; };
    static __device__ __forceinline__ Acc zero() { return Acc{f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}}; }
    // the format as panel_mma sees it (see PnF32).  One step = 32 columns of K: the planes h, l of the LDS block's fragment and of the
    // static one, three v_mfma_f32_16x16x32_f16.  Lds: plane stride `pstride`, RB images `img` apart (uint4)
    typedef uint4 Frag;
    struct AFrag { pn_f16x8 pl[NP]; };                          // (native vectors: copying HIP's uint4 inside a struct splits it into words)
    typedef AFrag BFrag;
    typedef const uint4* Stream;
    typedef uint4 LdsElem;
    struct Lds { int pstride, img; };
    static __device__ __forceinline__ Stream stream(const Frag* tile_base, int lane) { return tile_base + lane; }
    static __device__ __forceinline__ AFrag bits(const uint4* v) {
        AFrag f;
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) f.pl[pl] = __builtin_bit_cast(pn_f16x8, v[pl]);
        return f;
    }
    static __device__ __forceinline__ AFrag load_a(const LdsElem* sA, const Lds& l, int rb, int step, int lane) {
        uint4 v[NP];
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) v[pl] = sA[(size_t)rb * l.img + (size_t)pl * l.pstride + (size_t)step * 64 + lane];
        return bits(v);
    }
    static __device__ __forceinline__ BFrag load_b(Stream st, int step) {
        uint4 v[NP];
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) v[pl] = st[((size_t)step * NP + pl) * 64];
        return bits(v);
    }
    static __device__ __forceinline__ Acc step(const AFrag& a, const BFrag& b, Acc acc) {
#define PN2_MMA(dst, wp, ap) dst = __builtin_amdgcn_mfma_f32_16x16x32_f16(b.pl[wp], a.pl[ap], dst, 0, 0, 0)
        PN2_MMA(acc.l, 1, 0); PN2_MMA(acc.h, 0, 0); PN2_MMA(acc.l, 0, 1);
#undef PN2_MMA
        return acc;
    }
    static __device__ __forceinline__ f32x4_t value(const Acc& a, float row_isc, const f32x4_t& col_isc) {
        f32x4_t v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaf(a.l[r], 0x1p-11f, a.h[r]) * row_isc * col_isc[r];   // (powers of two: exact; one after the other: their product alone may leave fp32's range)
        return v;
    }
    static __device__ __forceinline__ float row_isc(const uint4* image, int pstride, int j) { return ((const float*)(image + (size_t)NP * pstride))[j]; }
    // the power of two that takes `bound` (>= every |a| of a row; 0: an all-zero row) into [2^13, 2^14), and its inverse
    static __device__ __forceinline__ void pow2(float bound, float& sc, float& isc) {
        const int se = bound == 0.f ? 127 : min(max(267 - (int)((__float_as_uint(bound) >> 23) & 255u), 4), 250);
        sc = __uint_as_float((unsigned)se << 23);
        isc = __uint_as_float((unsigned)(254 - se) << 23);
    }
    static __device__ __forceinline__ f32x4_t tile_isc(const PanelB3& B, int tile, int g);    // the lane's four columns 16 tile + 4 g ..
    // rows [m0, m0 + 16 RB) x columns [k0, k0 + kn) of A as RB images of two fp16 planes, each [kpad / 8 chunks][16 rows] x 16 bytes,
    // + the 16 inverse row scales behind each image's planes.  NT threads (a multiple of 64); contains ONE __syncthreads (every thread
    // of the workgroup must call); the caller's barrier after it publishes the images.  A thread's items all belong to row (tid & 15):
    // up to MAXIT items per image stay in registers between the maximum and the conversion, longer blocks are read twice.
    template <int NT, int RB, int MAXIT>
    static __device__ __forceinline__ void stage(uint4* __restrict__ lds, int img, const float* __restrict__ A, int lda, int m0, int M, int k0,
                                                 int kn, int kpad, int tid) {
        const int nch = kpad >> 3, nit = nch * 16, pstride = nit, wave = tid >> 6, lane = tid & 63, i = tid & 15;
        const bool vec = ((lda & 3) == 0) && ((k0 & 3) == 0) && ((((size_t)A) & 15) == 0);
        auto load8 = [&](int rb, int it, float* v) {
            const int ch = it >> 4, row = m0 + 16 * rb + i, k = 8 * ch;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
            if (row < M && k < kn) {
                const float* p = A + (size_t)row * lda + k0 + k;
                if (vec && k + 7 < kn) {
                    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
                    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) if (k + e < kn) v[e] = p[e];
                }
            }
        };
        auto amax8 = [&](const float* v, float m) {
#pragma unroll
            for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(v[e]));
            return m;
        };
        auto put = [&](int rb, int it, const float* v, float sc) {
            unsigned h[4], l[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x0 = v[2 * e] * sc, x1 = v[2 * e + 1] * sc;
                h[e] = pn2_pk2(x0, x1);
                const pn_f16x2 hh = __builtin_bit_cast(pn_f16x2, h[e]);
                l[e] = pn2_pk2((x0 - (float)hh[0]) * 2048.f, (x1 - (float)hh[1]) * 2048.f);
            }
            uint4* const im = lds + (size_t)rb * img;
            im[(size_t)0 * pstride + it] = make_uint4(h[0], h[1], h[2], h[3]);
            im[(size_t)1 * pstride + it] = make_uint4(l[0], l[1], l[2], l[3]);
        };
        const bool keep = nit <= MAXIT * NT;
        float kv[RB][MAXIT][8], mx[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) mx[rb] = 0.f;
        if (keep) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int n = 0; n < MAXIT; ++n) {
                    const int it = tid + n * NT;
                    if (it < nit) { load8(rb, it, kv[rb][n]); mx[rb] = amax8(kv[rb][n], mx[rb]); }
                }
        } else {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
                for (int it = tid; it < nit; it += NT) { float v[8]; load8(rb, it, v); mx[rb] = amax8(v, mx[rb]); }
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            float m = mx[rb];
            m = fmaxf(m, __shfl_xor(m, 16));
            m = fmaxf(m, __shfl_xor(m, 32));
            float* const sc = (float*)(lds + (size_t)rb * img + (size_t)NP * pstride);
            if (lane < 16) sc[16 + wave * 16 + lane] = m;
        }
        __syncthreads();
        float scl[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            float* const sc = (float*)(lds + (size_t)rb * img + (size_t)NP * pstride);
            float m = 0.f;
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) m = fmaxf(m, sc[16 + w * 16 + i]);
            float isc;                                          // the row's largest |a| -> [2^13, 2^14); an all-zero row keeps 1, the ends are clamped
            pow2(m, scl[rb], isc);
            if (tid < 16) sc[tid] = isc;
        }
        if (keep) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int n = 0; n < MAXIT; ++n) {
                    const int it = tid + n * NT;
                    if (it < nit) put(rb, it, kv[rb][n], scl[rb]);
                }
        } else {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
                for (int it = tid; it < nit; it += NT) { float v[8]; load8(rb, it, v); put(rb, it, v, scl[rb]); }
        }
    }
    static inline void pack(const float* src, long sk, long sn, int K, int N, std::vector<unsigned>& out, std::vector<float>& isc, int* ntile,
                            int* nst) {
        const int nt = (N + 15) / 16, ns = (K + 31) / 32;
        out.assign((size_t)nt * ns * NP * 64 * 4, 0u);
        isc.assign((size_t)nt * 16, 1.f);
        std::vector<float> scl((size_t)nt * 16, 1.f);
        for (int n = 0; n < N; ++n) {
            float mx = 0.f;
            for (int k = 0; k < K; ++k) mx = std::max(mx, fabsf(src[(long)k * sk + (long)n * sn]));
            int ex = 0;
            if (mx > 0.f && std::isfinite(mx)) { frexpf(mx, &ex); ex = std::min(std::max(14 - ex, -100), 100); }   // mx in [2^(ex-1), 2^ex) -> [2^13, 2^14)
            scl[(size_t)n] = ldexpf(1.f, ex);
            isc[(size_t)n] = ldexpf(1.f, -ex);
        }
        for (int t = 0; t < nt; ++t) {
            for (int s = 0; s < ns; ++s)
                for (int l = 0; l < 64; ++l) {
                    const int n = 16 * t + (l & 15);
                    if (n >= N) continue;
                    for (int e = 0; e < 8; ++e) {
                        const int k = 32 * s + 8 * (l >> 4) + e;
                        if (k >= K) continue;
                        const float x = src[(long)k * sk + (long)n * sn] * scl[(size_t)n];
                        const unsigned h = pn2_f16_host(x);
                        const unsigned lo = pn2_f16_host((x - pn2_f16f_host(h)) * 2048.f);
                        const unsigned part[2] = {h, lo};
                        for (int pl = 0; pl < NP; ++pl) {
                            unsigned& w = out[((((size_t)t * ns + s) * NP + pl) * 64 + l) * 4 + (e >> 1)];
                            w |= part[pl] << (16 * (e & 1));
                        }
                    }
                }
        }
        *ntile = nt;
        *nst = ns;
    }
};
// device form of PnH2::pack (r6), same arithmetic: the column scales (largest |B(., n)| -> [2^13, 2^14), all-zero / non-finite
// columns keep 1) by one of two kernels -- B row-major (sn == 1): a thread per column; B column-major (sk == 1): a workgroup per
// column -- then one thread per fragment lane writes its 16 bytes of each plane.  scl / isc: [16 ntile], padding columns 1.
__device__ __forceinline__ void pnh2_col_scale(float mx, float* scl, float* isc) {
    int ex = 0;
    if (mx > 0.f && mx < INFINITY) { (void)frexpf(mx, &ex); ex = min(max(14 - ex, -100), 100); }
    *scl = ldexpf(1.f, ex);
    *isc = ldexpf(1.f, -ex);
}
__global__ __launch_bounds__(256) void pnh2_colscale_rowmajor_kernel(const float* __restrict__ src, long sk, int K, int N, int npad,
                                                                     float* __restrict__ scl, float* __restrict__ isc) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= npad) return;
    float mx = 0.f;
    if (n < N) for (int k = 0; k < K; ++k) mx = fmaxf(mx, fabsf(src[(long)k * sk + n]));
    pnh2_col_scale(mx, scl + n, isc + n);
}
__global__ __launch_bounds__(256) void pnh2_colscale_colmajor_kernel(const float* __restrict__ src, long sn, int K, int N, int npad,
                                                                     float* __restrict__ scl, float* __restrict__ isc) {
    __shared__ float part[4];
    const int n = blockIdx.x;
    float mx = 0.f;
    if (n < N) for (int k = threadIdx.x; k < K; k += 256) mx = fmaxf(mx, fabsf(src[(long)n * sn + k]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) pnh2_col_scale(fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3])), scl + n, isc + n);
}
__global__ __launch_bounds__(256) void pnh2_pack_kernel(const float* __restrict__ src, long sk, long sn, int K, int N, int nt, int ns,
                                                        const float* __restrict__ scl, uint4* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)nt * ns * 64) return;
    const int l = (int)(idx & 63), s = (int)((idx >> 6) % ns), t = (int)((idx >> 6) / ns);
    const int n = 16 * t + (l & 15);
    unsigned h[4] = {0u, 0u, 0u, 0u}, lo[4] = {0u, 0u, 0u, 0u};
    if (n < N) {
        const float sc = scl[n];
        for (int e = 0; e < 8; ++e) {
            const int k = 32 * s + 8 * (l >> 4) + e;
            if (k >= K) continue;
            const float x = src[(long)k * sk + (long)n * sn] * sc;
            const _Float16 hh = (_Float16)x;
            const _Float16 ll = (_Float16)((x - (float)hh) * 2048.f);
            h[e >> 1] |= (unsigned)__builtin_bit_cast(unsigned short, hh) << (16 * (e & 1));
            lo[e >> 1] |= (unsigned)__builtin_bit_cast(unsigned short, ll) << (16 * (e & 1));
        }
    }
    uint4* const o = out + (((size_t)t * ns + s) * 2) * 64 + l;
    o[0] = make_uint4(h[0], h[1], h[2], h[3]);
    o[64] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

typedef PnH2 PnF;                                               // the format of the panel_gemm3_* family
__device__ __forceinline__ f32x4_t PnH2::tile_isc(const PanelB3& B, int tile, int g) { return ((const f32x4_t*)B.isc)[(size_t)min(tile, B.ntile - 1) * 4 + g]; }
constexpr int PNF = PnF::NP;
// uint4 per 16-row image of kpad columns; bytes of RB of them (fdc_forms.h, by plane count)
static_assert(PnH2::SC_U4 == PN_SC_U4, "fdc_forms.h sizes the LDS images");
constexpr __host__ __device__ int pnf_img_u4(int kpad) { return pn_img_u4(PNF, kpad); }
constexpr __host__ __device__ size_t pnf_lds_bytes(int kpad, int rb) { return pn_lds_bytes(PNF, kpad, rb); }

// a lane's four results of one tile: columns n4 .. n4 + 3 of row m
__device__ __forceinline__ void pnf_store4(float* __restrict__ C, int ldc, int N, int m, int n4, const f32x4_t v) {
    float* dst = C + (size_t)m * ldc + n4;
    if (n4 + 3 < N) *(f32x4u_t*)dst = f32x4u_t{v[0], v[1], v[2], v[3]};
    else {
#pragma unroll
        for (int r = 0; r < 4; ++r) if (n4 + r < N) dst[r] = v[r];
    }
}

// C[M, N] = A[M, K] x B on the split (same workgroup shape and XCD-aware map as panel_gemm_kernel<1>; K in one slab).
// Dynamic LDS: pnf_lds_bytes(kpad, 1) per row block.
// NW waves per workgroup = NW column tiles (r5; 8 until then).  A 128-frame shard's products ran on 96 (forward) and 32 (data
// gradient) workgroups of eight waves -- the gradient's 32 each pulled 1.1 MB of fragments through one CU's return path, 11.5 us
// for a product of 0.2 GFLOP; with fewer waves per workgroup there are enough workgroups for the chip (launcher: panel_gemm3).
template <int NW>
__global__ __launch_bounds__(64 * NW) void panel_gemm3_kernel(const float* __restrict__ A, int lda, int M, int K, PanelB3 B,
                                                          float* __restrict__ C, int ldc, int N, PnMap mp) {
    extern __shared__ __attribute__((aligned(16))) uint4 pn3_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const PnBlock pb = panel_block(mp);
    if (!pb.on) return;
    const int rbk = pb.rbk, cbk = pb.cbk;
    const int tile = cbk * NW + wave, m0 = rbk * 16;
    const bool active = tile < B.ntile;
    const int kpad = (K + 31) & ~31, nst = kpad >> 5, pstride = (kpad >> 3) * 16;
    PnRing<PnF, 1, 2> rg;
    panel_prefetch<PnF, 1, 2>(rg, {B.f + (size_t)(active ? tile : 0) * B.nst * PNF * 64}, nst, lane);      // in flight while the A block is staged
    const f32x4_t ts = PnF::tile_isc(B, tile, g);                // (with the first fragments: at the epilogue it would be a cold round trip of its own)
    PnF::stage<64 * NW, 1, (NW == 8 ? 6 : 4)>(pn3_lds, 0, A, lda, m0, M, 0, K, kpad, tid);
    __syncthreads();
    PnF::Acc acc = PnF::zero();
    if (active) panel_mma<PnF, 1, 1, 2, PnOrder::StaticPinLds>(pn3_lds, {pstride, 0}, rg, nst, &acc, lane);
    const int n4 = tile * 16 + 4 * g, m = m0 + j;
    if (active && n4 < N && m < M) pnf_store4(C, ldc, N, m, n4, PnF::value(acc, PnF::row_isc(pn3_lds, pstride, j), ts));
}
// Two row blocks per fragment stream, for clip-sized M.  s_memtime in panel_gemm3_kernel (1024 rows): the MFMA phase of the
// K = 1500 data gradient takes 20.8 k cycles for 282 MFMAs per wave -- 74 cycles each where the pipe needs 16 -- and its eight
// waves receive 8 x 141 KB of fragments in that time: 54 bytes per clock, against the 64 a CU's vector-memory path returns.
// The bound is that return path (L1 hit or not: streaming one tile to all eight waves changed nothing), so what helps is
// fewer fragment bytes per MFMA: every fragment multiplies TWO 16-row blocks.  Twelve waves = twelve column tiles per
// workgroup, 32 rows, both images in LDS (K <= 768); column group = blockIdx & 7 = XCD, so each
// XCD streams its own eighth of the static operand.  Grid: 8 x ceil(M / 32) workgroups (256 at 1024 rows: one per CU).
__global__ __launch_bounds__(768) void panel_gemm3_rb2_kernel(const float* __restrict__ A, int lda, int M, int K, PanelB3 B,
                                                              float* __restrict__ C, int ldc, int N) {
    extern __shared__ __attribute__((aligned(16))) uint4 pn3_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const int xcd = blockIdx.x & 7, m0 = (int)(blockIdx.x >> 3) * 32;
    const int ncb = (B.ntile + 11) / 12, cpg = (ncb + 7) / 8;            // column blocks of 12 tiles; per XCD
    const int kpad = (K + 31) & ~31, nst = kpad >> 5, pstride = (kpad >> 3) * 16, img = pnf_img_u4(kpad);
    if (xcd * cpg >= ncb) return;
    PnRing<PnF, 1, 2> rg;
    panel_prefetch<PnF, 1, 2>(rg, {B.f + (size_t)min((xcd * cpg) * 12 + wave, B.ntile - 1) * B.nst * PNF * 64}, nst, lane);
    f32x4_t ts = PnF::tile_isc(B, (xcd * cpg) * 12 + wave, g);   // (requested with the fragments: see panel_gemm3_kernel)
    PnF::stage<768, 2, 2>(pn3_lds, img, A, lda, m0, M, 0, K, kpad, tid);
    __syncthreads();
    const float rs[2] = {PnF::row_isc(pn3_lds, pstride, j), PnF::row_isc(pn3_lds + img, pstride, j)};
    for (int cb = xcd * cpg; cb < min(ncb, (xcd + 1) * cpg); ++cb) {
        const int tile = cb * 12 + wave;
        PnF::Acc acc[2] = {PnF::zero(), PnF::zero()};
        if (tile < B.ntile) panel_mma<PnF, 2, 1, 2, PnOrder::StaticPinLds>(pn3_lds, {pstride, img}, rg, nst, acc, lane);
        const f32x4_t tsc = ts;
        if (cb + 1 < min(ncb, (xcd + 1) * cpg)) {
            panel_prefetch<PnF, 1, 2>(rg, {B.f + (size_t)min((cb + 1) * 12 + wave, B.ntile - 1) * B.nst * PNF * 64}, nst, lane);
            ts = PnF::tile_isc(B, (cb + 1) * 12 + wave, g);
        }
        const int n4 = tile * 16 + 4 * g;
        if (tile < B.ntile && n4 < N) {
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                const int m = m0 + 16 * rb + j;
                if (m < M) pnf_store4(C, ldc, N, m, n4, PnF::value(acc[rb], rs[rb], tsc));
            }
        }
    }
}

// ... and for long K (the data gradient, K = 1500: two images of all of K do not fit) each workgroup takes HALF of K for two
// row blocks and leaves a partial product: C = Cpart[0] + Cpart[1], added by the consumer.  XCD = blockIdx & 7 =
// (K half, column block of 8 tiles): each XCD streams its own eighth of the static operand; slot = blockIdx >> 3 = row pair.
// N <= 32 tiles (four column blocks), kpad / 2 rounded up to a step <= 768 columns per half.  Grid 8 x ceil(M / 32).
__global__ __launch_bounds__(512) void panel_gemm3_rb2k_kernel(const float* __restrict__ A, int lda, int M, int K, PanelB3 B,
                                                               float* __restrict__ Cpart, size_t part_stride, int ldc, int N) {
    extern __shared__ __attribute__((aligned(16))) uint4 pn3_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const int xcd = blockIdx.x & 7, half = xcd >> 2, cb = xcd & 3, m0 = (int)(blockIdx.x >> 3) * 32;
    const int nst_all = (K + 31) >> 5, s0 = half ? (nst_all + 1) / 2 : 0, s1 = half ? nst_all : (nst_all + 1) / 2;
    const int nst = s1 - s0, kpad = 32 * nst, k0 = 32 * s0, kn = min(K, 32 * s1) - k0;
    const int pstride = (kpad >> 3) * 16, img = pnf_img_u4(kpad);
    const int tile = cb * 8 + wave;
    const bool active = tile < B.ntile && nst > 0;
    PnRing<PnF, 1, 2> rg;
    panel_prefetch<PnF, 1, 2>(rg, {B.f + ((size_t)(active ? tile : 0) * B.nst + s0) * PNF * 64}, max(nst, 1), lane);
    const f32x4_t ts = PnF::tile_isc(B, tile, g);               // (requested with the fragments: see panel_gemm3_kernel)
    PnF::stage<512, 2, 3>(pn3_lds, img, A, lda, m0, M, k0, kn, kpad, tid);
    __syncthreads();
    PnF::Acc acc[2] = {PnF::zero(), PnF::zero()};
    if (active) panel_mma<PnF, 2, 1, 2, PnOrder::StaticPinLds>(pn3_lds, {pstride, img}, rg, nst, acc, lane);
    const int n4 = tile * 16 + 4 * g;
    if (tile < B.ntile && n4 < N) {
        float* const C = Cpart + (size_t)half * part_stride;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const int m = m0 + 16 * rb + j;
            if (m < M) pnf_store4(C, ldc, N, m, n4, PnF::value(acc[rb], PnF::row_isc(pn3_lds + (size_t)rb * img, pstride, j), ts));
        }
    }
}
static inline hipError_t panel_gemm3_rb2k(const PanelPlan& pl, const float* A, int lda, int M, int K, const PanelB3& B, float* Cpart, size_t part_stride,
                                          int ldc, int N, hipStream_t st) {
    note_form(form_name(pl.form));
    hipLaunchKernelGGL(panel_gemm3_rb2k_kernel, dim3(pl.grid), dim3(pl.block), pl.lds, st, A, lda, M, K, B, Cpart, part_stride, ldc, N);
    return hipGetLastError();
}

// wide outputs on the split: the column-walking form of panel_gemm_wide_kernel (A staged once per workgroup, all the
// column blocks of the XCD's share walked; next block's fragments requested before the stores)
template <int RB>
__global__ __launch_bounds__(512) void panel_gemm3_wide_kernel(const float* __restrict__ A, int lda, int M, int K, PanelB3 B,
                                                               float* __restrict__ C, int ldc, int N, int cs) {
    // cs (r5): an XCD's share of the column blocks is cut into cs parts, one workgroup each per row block -- grid 8 x row blocks x cs.
    // With cs = 1 a 512-row product (BASELINE config 5) ran on 128 workgroups and a 128-row shard of it on 32: every workgroup
    // walks an eighth of the 93 MB operand through ONE CU's 64 B / clock, 205-214 us whatever M is (profiles/r5_c5_*).
    extern __shared__ __attribute__((aligned(16))) uint4 pn3_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const int nrb = (M + 16 * RB - 1) / (16 * RB);
    const int xcd = blockIdx.x & 7, slot = (int)(blockIdx.x >> 3), m0 = (slot % nrb) * (16 * RB), part = slot / nrb;
    const int ncb = (B.ntile + 7) / 8, cpg = (ncb + 7) / 8;
    const int xb0 = xcd * cpg, xb1 = min(ncb, xb0 + cpg), per = (max(xb1 - xb0, 0) + cs - 1) / cs;
    const int cb0 = xb0 + part * per, cb1 = min(xb1, cb0 + per);
    const int kpad = (K + 31) & ~31, nst = kpad >> 5, pstride = (kpad >> 3) * 16, img = pnf_img_u4(kpad);
    if (cb0 >= cb1) return;
    PnRing<PnF, 1, 2> rg;
    panel_prefetch<PnF, 1, 2>(rg, {B.f + (size_t)min(cb0 * 8 + wave, B.ntile - 1) * B.nst * PNF * 64}, nst, lane);
    f32x4_t ts = PnF::tile_isc(B, cb0 * 8 + wave, g);           // (requested with the fragments: see panel_gemm3_kernel)
    PnF::stage<512, RB, 3>(pn3_lds, img, A, lda, m0, M, 0, K, kpad, tid);
    __syncthreads();
    float rs[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) rs[rb] = PnF::row_isc(pn3_lds + (size_t)rb * img, pstride, j);
    for (int cb = cb0; cb < cb1; ++cb) {
        const int tile = cb * 8 + wave;
        PnF::Acc acc[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) acc[rb] = PnF::zero();
        if (tile < B.ntile) panel_mma<PnF, RB, 1, 2, PnOrder::StaticPinLds>(pn3_lds, {pstride, img}, rg, nst, acc, lane);
        const f32x4_t tsc = ts;
        if (cb + 1 < cb1) {
            panel_prefetch<PnF, 1, 2>(rg, {B.f + (size_t)min((cb + 1) * 8 + wave, B.ntile - 1) * B.nst * PNF * 64}, nst, lane);
            ts = PnF::tile_isc(B, (cb + 1) * 8 + wave, g);
        }
        const int n4 = tile * 16 + 4 * g;
        if (tile < B.ntile && n4 < N) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int m = m0 + 16 * rb + j;
                if (m < M) pnf_store4(C, ldc, N, m, n4, PnF::value(acc[rb], rs[rb], tsc));
            }
        }
    }
}

// executes a plan of plan_panel3 (fdc_forms.h): all of K in one LDS image
static inline hipError_t panel_gemm3(const float* A, int lda, int M, int K, const PanelB3& B, float* C, int ldc, int N, hipStream_t st) {
    if (M <= 0 || N <= 0) return hipSuccess;
    const PanelPlan pl = plan_panel3(M, K, B.ntile, B.nst, PNF, proc_switches());
    const dim3 grid(pl.grid), block(pl.block);
    if (pl.form != F_NONE) note_form(form_name(pl.form));
    switch (pl.form) {
    case F_PANEL3_WIDE: hipLaunchKernelGGL(panel_gemm3_wide_kernel<2>, grid, block, pl.lds, st, A, lda, M, K, B, C, ldc, N, pl.cs); break;
    case F_PANEL3_RB2: hipLaunchKernelGGL(panel_gemm3_rb2_kernel, grid, block, pl.lds, st, A, lda, M, K, B, C, ldc, N); break;
    case F_PANEL3:
        if (pl.nw == 8) hipLaunchKernelGGL(panel_gemm3_kernel<8>, grid, block, pl.lds, st, A, lda, M, K, B, C, ldc, N, pl.mp);
        else if (pl.nw == 4) hipLaunchKernelGGL(panel_gemm3_kernel<4>, grid, block, pl.lds, st, A, lda, M, K, B, C, ldc, N, pl.mp);
        else hipLaunchKernelGGL(panel_gemm3_kernel<2>, grid, block, pl.lds, st, A, lda, M, K, B, C, ldc, N, pl.mp);
        break;
    default: return hipErrorInvalidValue;                  // K beyond one image: callers fall back to panel_gemm (K slabs)
    }
    return hipGetLastError();
}

// Wide outputs (the full-mesh blend: N = 3 V = 31 425 columns, B = 62 MB): a workgroup keeps its 16 RB rows of A in LDS and
// walks ALL the column blocks of its XCD's share of B, so A is staged once per workgroup instead of once per (row, column)
// block (measured with one column block per workgroup: staging 14.7 k of a 45 k-cycle lifetime, exposed because the 127 KB
// image leaves room for one workgroup per CU) and the workgroups of an XCD stream the same column blocks at the same
// time: each slice of B crosses the fabric once.  The next column block's first fragments are requested before the
// current block's stores.  K must fit one slab.  Grid: 8 * ceil(M / (16 RB)) workgroups, blockIdx & 7 = XCD = column share.
template <int RB>
__global__ __launch_bounds__(512) void panel_gemm_wide_kernel(const float* __restrict__ A, int lda, int M, int K, PanelB B,
                                                              float* __restrict__ C, int ldc, int N) {
    extern __shared__ __attribute__((aligned(16))) float pn_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const int xcd = blockIdx.x & 7, m0 = (int)(blockIdx.x >> 3) * (16 * RB);
    const int ncb = (B.ntile + 7) / 8, cpg = (ncb + 7) / 8;
    const int cb0 = xcd * cpg, cb1 = min(ncb, cb0 + cpg);
    const int kpad = (K + 15) & ~15, nss = kpad >> 4, img = kpad * 16;
    if (cb0 >= cb1) return;
    PN_STAMP(0);
    PnRing<PnF32, 1, 4> rg;
    {
        const int t0 = min(cb0 * 8 + wave, B.ntile - 1);
        const float4* bfp = B.f + (size_t)t0 * B.nss * 64;
        panel_prefetch<PnF32, 1, 4>(rg, {bfp}, nss, lane);
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) panel_stage<512>(pn_lds + (size_t)rb * img, A, lda, m0 + 16 * rb, M, 0, K, kpad, tid);
    __syncthreads();
    PN_STAMP(1);
    for (int cb = cb0; cb < cb1; ++cb) {
        if (cb == cb0 + 1) PN_STAMP(2);
        const int tile = cb * 8 + wave;
        f32x4_t acc[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) acc[rb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (tile < B.ntile) panel_mma<PnF32, RB, 1, 4, PnOrder::StaticPinLds>(pn_lds, {img}, rg, nss, acc, lane);
        if (cb + 1 < cb1) {                                          // next block's first fragments: in flight during the stores
            const int tn = min((cb + 1) * 8 + wave, B.ntile - 1);
            const float4* bfp = B.f + (size_t)tn * B.nss * 64;
            panel_prefetch<PnF32, 1, 4>(rg, {bfp}, nss, lane);
        }
        const int n4 = tile * 16 + 4 * g;
        if (tile < B.ntile && n4 < N) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int m = m0 + 16 * rb + j;
                if (m < M) {
                    float* dst = C + (size_t)m * ldc + n4;
                    if (n4 + 3 < N) *(f32x4u_t*)dst = f32x4u_t{acc[rb][0], acc[rb][1], acc[rb][2], acc[rb][3]};
                    else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) if (n4 + r < N) dst[r] = acc[rb][r];
                    }
                }
            }
        }
    }
    PN_STAMP(3);
}

static inline hipError_t panel_gemm(const float* A, int lda, int M, int K, const PanelB& B, float* C, int ldc, int N, hipStream_t st) {
    if (M <= 0 || N <= 0) return hipSuccess;
    // one row block per workgroup while an XCD's slice of the operand stays inside its L2 (the loop's products: a 3 MB panel);
    // wide outputs (full-mesh blend, N = 31 425) take the column-walking form with two row blocks per fragment stream
    const size_t b_bytes = (size_t)B.ntile * B.nss * 1024;
    const int kpad = (K + 15) & ~15;
    const int ncb = (B.ntile + 7) / 8;
    if (b_bytes > (size_t)(24u << 20) && M >= 32 && kpad <= 1024) {
        hipLaunchKernelGGL(panel_gemm_wide_kernel<2>, dim3(8 * ((M + 31) / 32)), dim3(512), (size_t)2 * kpad * 16 * sizeof(float), st, A, lda, M, K,
                           B, C, ldc, N);
    } else {
        const int kslab = kpad <= 1536 ? kpad : 1024;               // <= 96 KiB
        const PnMap mp = panel_map((M + 15) / 16, ncb, (size_t)M * K * 4, b_bytes);
        hipLaunchKernelGGL(panel_gemm_kernel<1>, dim3(8 * mp.rpg * mp.cpg), dim3(512), (size_t)kslab * 16 * sizeof(float), st, A, lda, M, K, B,
                           kslab, C, ldc, N, mp);
    }
    return hipGetLastError();
}

// Long K, few rows (r5: the data gradient [M,1500] x [1500,496] of a SHARD, M = 128..383 -- too few rows for the two-K-halves form,
// and as a plain one-row-block product 32 workgroups that each pull 1.1 MB of fragments through one CU: 15 us for 0.2 GFLOP).  K is
// split over the EIGHT WAVES of a workgroup: every wave streams its eighth of K for the workgroup's T column tiles, the eight partial
// tiles meet in LDS and are added in wave order -- one output, no partial products in global memory, M / 16 x tiles / T workgroups.
template <int T>
__global__ __launch_bounds__(512) void panel_gemm3_ksw_kernel(const float* __restrict__ A, int lda, int M, int K, PanelB3 B,
                                                              float* __restrict__ C, int ldc, int N, PnMap mp) {
    extern __shared__ __attribute__((aligned(16))) uint4 pn3_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const PnBlock pb = panel_block(mp);
    if (!pb.on) return;
    const int rbk = pb.rbk, cbk = pb.cbk;
    const int tile0 = cbk * T, m0 = rbk * 16;
    const int kpad = (K + 31) & ~31, nst_all = kpad >> 5, pstride = (kpad >> 3) * 16;
    const int per = (nst_all + 7) >> 3, s_lo = min(nst_all, wave * per), nst = min(nst_all, s_lo + per) - s_lo;
    PnRing<PnF, T, 2> rg;
    if (nst > 0) {                                             // (wave-uniform) in flight while the A block is staged
        const uint4* bf[T];
#pragma unroll
        for (int t = 0; t < T; ++t) bf[t] = B.f + ((size_t)min(tile0 + t, B.ntile - 1) * B.nst + s_lo) * PNF * 64;
        panel_prefetch<PnF, T, 2>(rg, bf, nst, lane);
    }
    f32x4_t ts[T];
#pragma unroll
    for (int t = 0; t < T; ++t) ts[t] = PnF::tile_isc(B, tile0 + t, g);
    PnF::stage<512, 1, 6>(pn3_lds, 0, A, lda, m0, M, 0, K, kpad, tid);
    __syncthreads();
    PnF::Acc acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = PnF::zero();
    if (nst > 0) panel_mma<PnF, 1, T, 2, PnOrder::LdsStaticPin>(pn3_lds + (size_t)s_lo * 64, {pstride, 0}, rg, nst, acc, lane);
    const float rs = PnF::row_isc(pn3_lds, pstride, j);        // (behind the planes: the meeting place below does not reach it)
    __syncthreads();                                           // every wave is done with the image: its head becomes the meeting place
    float4* const red = (float4*)pn3_lds;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const f32x4_t v = PnF::value(acc[t], rs, ts[t]);
        red[(size_t)(wave * T + t) * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
    if (wave < T) {                                            // wave t adds tile t's eight parts in wave order
        float4 sum = red[(size_t)wave * 64 + lane];
#pragma unroll
        for (int w = 1; w < 8; ++w) {
            const float4 v = red[(size_t)(w * T + wave) * 64 + lane];
            sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
        }
        const int tile = tile0 + wave, n4 = tile * 16 + 4 * g, m = m0 + j;
        if (tile < B.ntile && n4 < N && m < M) pnf_store4(C, ldc, N, m, n4, f32x4_t{sum.x, sum.y, sum.z, sum.w});
    }
}
static inline hipError_t panel_gemm3_ksw(const PanelPlan& pl, const float* A, int lda, int M, int K, const PanelB3& B, float* C, int ldc, int N, hipStream_t st) {
    if (M <= 0 || N <= 0) return hipSuccess;
    static std::atomic<uint64_t> attr{0};                      // per DEVICE: the attribute belongs to one device's code object
    const hipError_t e = fdc_allow_lds(attr, pl.max_lds, {(const void*)panel_gemm3_ksw_kernel<2>, (const void*)panel_gemm3_ksw_kernel<1>});
    if (e != hipSuccess) return e;
    note_form(form_name(pl.form));
    if (pl.T == 2)
        hipLaunchKernelGGL(panel_gemm3_ksw_kernel<2>, dim3(pl.grid), dim3(pl.block), pl.lds, st, A, lda, M, K, B, C, ldc, N, pl.mp);
    else
        hipLaunchKernelGGL(panel_gemm3_ksw_kernel<1>, dim3(pl.grid), dim3(pl.block), pl.lds, st, A, lda, M, K, B, C, ldc, N, pl.mp);
    return hipGetLastError();
}

// ... and for K far beyond any LDS image (r5: the FULL mesh's data gradient, K = 3 V = 31 425 -- BASELINE config 5's contact set, mode
// 'local', the body-model operator's backward; it ran on the generic fp32 tiles, 387 us at 512 rows and 214 us at 128): K in `ks`
// parts, a workgroup = (part, column block of 8 tiles, row pair) walks its part slab by slab -- stage the slab's two 16-row images,
// stream the slab's fragments, accumulate in registers -- and leaves one partial product; panel_part_sum_kernel adds the parts in
// ascending order.  Workgroup b: role = b % (ks ncb) = (part, column block) -> consecutive workgroups = consecutive roles, so with
// ks ncb a multiple of 8 an XCD keeps streaming the same eighth of the static operand; row pair = b / (ks ncb).
template <int RB, int T>
__global__ __launch_bounds__(512) void panel_gemm3_kloop_kernel(const float* __restrict__ A, int lda, int M, int K, PanelB3 B,
                                                                float* __restrict__ Cpart, size_t part_stride, int ldc, int N, int ks,
                                                                int slab_steps) {
    extern __shared__ __attribute__((aligned(16))) uint4 pn3_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const int ncb = (B.ntile + 8 * T - 1) / (8 * T), nrole = ks * ncb;
    const int role = (int)blockIdx.x % nrole, m0 = ((int)blockIdx.x / nrole) * (16 * RB), part = role / ncb, cb = role % ncb;
    const int nst_all = (K + 31) >> 5, per = (nst_all + ks - 1) / ks, s_lo = part * per, s_hi = min(nst_all, s_lo + per);
    const int tile0 = (cb * 8 + wave) * T;                      // this wave's T consecutive column tiles
    const int kpad = 32 * slab_steps, pstride = (kpad >> 3) * 16, img = pnf_img_u4(kpad);
    f32x4_t tot[RB * T];                                        // the slabs' products at the tile's scale (a row's scale is per slab)
#pragma unroll
    for (int i = 0; i < RB * T; ++i) tot[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    PnF::Acc acc[RB * T];
#pragma unroll
    for (int i = 0; i < RB * T; ++i) acc[i] = PnF::zero();
    f32x4_t ts[T];
#pragma unroll
    for (int t = 0; t < T; ++t) ts[t] = PnF::tile_isc(B, tile0 + t, g);
    for (int s0 = s_lo; s0 < s_hi; s0 += slab_steps) {
        const int nst = min(slab_steps, s_hi - s0), k0 = 32 * s0, kn = min(K, 32 * (s0 + nst)) - k0;
        PnRing<PnF, T, 2> rg;                                 // (requested before the staging: the first round trip hides behind it)
        const uint4* bf[T];
#pragma unroll
        for (int t = 0; t < T; ++t) bf[t] = B.f + ((size_t)min(tile0 + t, B.ntile - 1) * B.nst + s0) * PNF * 64;
        panel_prefetch<PnF, T, 2>(rg, bf, nst, lane);
        if (s0 > s_lo) __syncthreads();                         // every wave is done with the previous slab's images
        PnF::stage<512, RB, 3>(pn3_lds, img, A, lda, m0, M, k0, kn, kpad, tid);
        __syncthreads();
        if (tile0 < B.ntile) panel_mma<PnF, RB, T, 2, PnOrder::LdsStaticPin>(pn3_lds, {pstride, img}, rg, nst, acc, lane);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {                       // fold the slab in at its rows' scales
            const float rs = PnF::row_isc(pn3_lds + (size_t)rb * img, pstride, j);
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const f32x4_t v = PnF::value(acc[rb * T + t], rs, f32x4_t{1.f, 1.f, 1.f, 1.f});
#pragma unroll
                for (int r = 0; r < 4; ++r) tot[rb * T + t][r] += v[r];
                acc[rb * T + t] = PnF::zero();
            }
        }
    }
    float* const C = Cpart + (size_t)part * part_stride;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int n4 = (tile0 + t) * 16 + 4 * g;
        if (tile0 + t < B.ntile && n4 < N) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int m = m0 + 16 * rb + j;
                if (m < M) {
                    f32x4_t v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = tot[rb * T + t][r] * ts[t][r];
                    pnf_store4(C, ldc, N, m, n4, v);
                }
            }
        }
    }
}
__global__ void panel_part_sum_kernel(const float* __restrict__ part, int ks, size_t part_stride, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int p = 1; p < ks; ++p) s += part[(size_t)p * part_stride + i];
    out[i] = s;
}
// C [M rows of ldc] = sum of the parts; `part` must hold pl.ks x M x ldc floats
static inline hipError_t panel_gemm3_kloop(const PanelPlan& pl, const float* A, int lda, int M, int K, const PanelB3& B, float* part, float* C, int ldc, int N,
                                           hipStream_t st) {
    if (M <= 0 || N <= 0) return hipSuccess;
    constexpr int rb = PN3_KLOOP_RB, T = PN3_KLOOP_T;
    const size_t stride = (size_t)M * ldc;
    static std::atomic<uint64_t> attr{0};                      // per DEVICE: the attribute belongs to one device's code object
    const hipError_t e = fdc_allow_lds(attr, pl.max_lds, {(const void*)panel_gemm3_kloop_kernel<rb, T>});
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((panel_gemm3_kloop_kernel<rb, T>), dim3(pl.grid), dim3(pl.block), pl.lds, st, A, lda, M, K, B, part, stride, ldc, N, pl.ks, PN3_KLOOP_SLAB);
    note_form(form_name(pl.form));
    hipLaunchKernelGGL(panel_part_sum_kernel, dim3((unsigned)((stride + 255) / 256)), dim3(256), 0, st, part, pl.ks, stride, stride, C);
    return hipGetLastError();
}

// four consecutive columns n4 .. n4 + 3 of frame row j -> the planes of an LDS block (8 bytes per plane); sc: the row's scale
__device__ __forceinline__ void pnf_lds_store4(uint4* __restrict__ sA, int pstride, int n4, int j, float4 v, float sc) {
    const float x[4] = {v.x * sc, v.y * sc, v.z * sc, v.w * sc};
    unsigned h[2], l[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        h[e] = pn2_pk2(x[2 * e], x[2 * e + 1]);
        const pn_f16x2 hh = __builtin_bit_cast(pn_f16x2, h[e]);
        l[e] = pn2_pk2((x[2 * e] - (float)hh[0]) * 2048.f, (x[2 * e + 1] - (float)hh[1]) * 2048.f);
    }
    const size_t it = (size_t)(n4 >> 3) * 16 + j;
    const int half = (n4 >> 2) & 1;
    ((uint2*)(sA + (size_t)0 * pstride + it))[half] = make_uint2(h[0], h[1]);
    ((uint2*)(sA + (size_t)1 * pstride + it))[half] = make_uint2(l[0], l[1]);
}
// one latent value per thread (row i = tid >> 5, column k = tid & 31) straight into a 32-column image (plane stride `pstride`)
#define PN_DPP_MAX(m, ctrl) fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), ctrl, 0xF, 0xF, false)))
__device__ __forceinline__ void pnf_put_latent(uint4* __restrict__ sZ, int pstride, int i, int k, float v) {
    // the row's largest |z|: its 32 values sit in one half of a wave -- four DPP steps inside each row of 16 lanes, one exchange between rows
    float m = fabsf(v);
    m = PN_DPP_MAX(m, 0xB1);                                     // quad_perm [1,0,3,2]
    m = PN_DPP_MAX(m, 0x4E);                                     // quad_perm [2,3,0,1]
    m = PN_DPP_MAX(m, 0x141);                                    // row_half_mirror
    m = PN_DPP_MAX(m, 0x140);                                    // row_mirror
    m = fmaxf(m, __shfl_xor(m, 16));
    float sc, isc;
    PnH2::pow2(m, sc, isc);
    const float x = v * sc;
    const _Float16 h = (_Float16)x;
    const _Float16 l = (_Float16)((x - (float)h) * 2048.f);
    unsigned short* const img = (unsigned short*)sZ;
    const int it = (k >> 3) * 16 + i, e = k & 7;
    img[(size_t)(0 * pstride + it) * 8 + e] = __builtin_bit_cast(unsigned short, h);
    img[(size_t)(1 * pstride + it) * 8 + e] = __builtin_bit_cast(unsigned short, l);
    if (k == 0) ((float*)(sZ + (size_t)PnH2::NP * pstride))[i] = isc;
}
#undef PN_DPP_MAX

// ---------------------------------------------------------------------------------------------------------------------
// VPoser decoder (fc1 32 -> 512, LeakyReLU(0.2), fc2 512 -> 512, LeakyReLU(0.2), out 512 -> 126)
constexpr int VP_Z = 32, VP_H = 512, VP_NQ = 4, VP_QW = VP_H / VP_NQ;
struct VPoserPanels {
    PanelB w1, w2, w3;          // forward:  B(k, n) = W[n][k]   (y = x W^T + b)
    PanelB w3t, w2t, w1t;       // backward: B(k, n) = W[k][n]   (dx = dy W)
    const float *b1 = nullptr, *b2 = nullptr, *b3 = nullptr;
};

__device__ __forceinline__ float vp_lrelu(float v) { return v > 0.f ? v : 0.2f * v; }

// dX[row, latent columns] += ((p0 + p1) + (p2 + p3))   (the order the Adam kernel uses when it folds the partials itself)
__device__ __forceinline__ float vp_sum_dz(const float* __restrict__ part, size_t part_stride, size_t e) {
    return (part[e] + part[part_stride + e]) + (part[2 * part_stride + e] + part[3 * part_stride + e]);
}

// DeferredStep (fdc_loss.h), decoder side: element (row r0 + tid / 32, latent column tid % 32) of the 16 x 32 block AFTER the
// pending Adam step -- one element per thread of the 512-thread workgroup, rows >= row_hi zero.  Nothing is written back: the
// four quarter-workgroups of a row block all do this, pose_fwd_kernel repeats it for its row and stores parameters and moments.
__device__ __forceinline__ float vp_deferred_latent(const DeferredStep& ds, int r0, int row_hi, int tid) {
    const int i = tid >> 5, col = tid & 31, row = r0 + i;
    float pp = 0.f;
    if (row < row_hi) {
        const size_t e = (size_t)(row - ds.row0) * XDIM + X_LATENT + col;
        float mm = ds.x.m[e], vv = ds.x.v[e], gg = ds.x.g[e];
        pp = ds.x.p[e];
        if (ds.dzpart) gg += vp_sum_dz(ds.dzpart, ds.dz_stride, (size_t)row * VP_Z + col);
        adam_update(pp, mm, vv, gg, ds.x.a);
    }
    return pp;
}

// grid = 4 * ceil(rows / 16): blockIdx & 3 = hidden-column quarter q (blocks of one quarter share an XCD's L2: the
// dispatcher deals consecutive blocks to the 8 XCDs, so XCD x only ever streams quarter x & 3 of W2), blockIdx >> 2 = row block.
// Z = X + latent column (row stride ldx); rows [row_lo, row_hi).  H1, H2 [*, 512] (kept for the backward's masks),
// Opart [4][part_stride]: partial decoder outputs (row-major [*, 126]); the bias rides on partial 0.
// A launch may cover TWO row ranges (a shard's halo rows on either side of its owned rows, VpRows): row blocks [0, nb1) belong to
// [row_lo, row_hi), the rest to [row2_lo, row2_hi).  A row's result does not depend on the block it is decoded in.
struct VpRows { int nb1 = 0x7fffffff, row2_lo = 0, row2_hi = 0; };
__global__ __launch_bounds__(512) void vposer_fwd_fused_kernel(VPoserPanels P, const float* __restrict__ Z, int ldx, int row_lo,
                                                               int row_hi, float* __restrict__ H1, float* __restrict__ H2,
                                                               float* __restrict__ Opart, size_t part_stride, VpRows two, DeferredStep ds) {
    __shared__ __attribute__((aligned(16))) float lds[VP_Z * 16 + VP_H * 16 + VP_QW * 16];
    float* const sZ = lds;
    float* const sH1 = lds + VP_Z * 16;
    float* const sH2 = sH1 + VP_H * 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    int rblk = (int)(blockIdx.x >> 2);
    if (rblk >= two.nb1) { rblk -= two.nb1; row_lo = two.row2_lo; row_hi = two.row2_hi; }
    const int q = blockIdx.x & 3, r0 = row_lo + rblk * 16;
    PN_STAMP(0);
    PnRing<PnF32, 1, 4> rg2, rg3;                             // next layer's first fragments are requested before the barrier in front of it
    // all three layers' biases before the first barrier (see vposer_fwd_split3_kernel)
    float4 bias1[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) bias1[t] = *(const float4*)(P.b1 + (wave * 4 + t) * 16 + 4 * g);
    const float4 bias2 = *(const float4*)(P.b2 + (q * 8 + wave) * 16 + 4 * g);
    float bias3[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) bias3[e] = P.b3[min(wave * 16 + 4 * g + e, ODIM - 1)];
    {   // layer 1, all 512 columns (four tiles per wave)
        f32x4_t acc[4];
        const float4* bf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f}; bf[t] = P.w1.f + (size_t)(wave * 4 + t) * P.w1.nss * 64; }
        PnRing<PnF32, 4, 2> rg1;
        panel_prefetch<PnF32, 4, 2>(rg1, bf, VP_Z / 16, lane);
        if (ds.on) {                                       // (wave-uniform) the latent rows after the pending optimiser step,
            const int i = tid >> 5, k = tid & 31;          // straight into panel_stage's k-blocked image: [k / 4][row][k % 4]
            sZ[((k >> 2) * 16 + i) * 4 + (k & 3)] = vp_deferred_latent(ds, r0, row_hi, tid);
        } else
            panel_stage<512>(sZ, Z, ldx, r0, row_hi, 0, VP_Z, VP_Z, tid);
        __syncthreads();
        PN_STAMP(1);
        panel_mma<PnF32, 1, 4, 2, PnOrder::LdsTilePin>(sZ, {0}, rg1, VP_Z / 16, acc, lane);
        {
            const float4* bf2 = P.w2.f + (size_t)(q * 8 + wave) * P.w2.nss * 64;
            panel_prefetch<PnF32, 1, 4>(rg2, {bf2}, VP_H / 16, lane);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n4 = (wave * 4 + t) * 16 + 4 * g;
            const float4 bias = bias1[t];
            const float4 v = make_float4(vp_lrelu(acc[t][0] + bias.x), vp_lrelu(acc[t][1] + bias.y), vp_lrelu(acc[t][2] + bias.z),
                                         vp_lrelu(acc[t][3] + bias.w));
            *(float4*)(sH1 + (size_t)((n4 >> 2) * 16 + j) * 4) = v;
            if ((n4 / VP_QW) == q && r0 + j < row_hi) *(float4*)(H1 + (size_t)(r0 + j) * VP_H + n4) = v;
        }
    }
    __syncthreads();
    PN_STAMP(2);
    {   // layer 2, this quarter's 128 columns (one tile per wave)
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        const int tile = q * 8 + wave;
        panel_mma<PnF32, 1, 1, 4, PnOrder::LdsTilePin>(sH1, {0}, rg2, VP_H / 16, &acc, lane);
        {
            const float4* bf3 = P.w3.f + ((size_t)wave * P.w3.nss + q * (VP_QW / 16)) * 64;
            panel_prefetch<PnF32, 1, 4>(rg3, {bf3}, VP_QW / 16, lane);
        }
        const int n4 = tile * 16 + 4 * g;
        const float4 bias = bias2;
        const float4 v = make_float4(vp_lrelu(acc[0] + bias.x), vp_lrelu(acc[1] + bias.y), vp_lrelu(acc[2] + bias.z), vp_lrelu(acc[3] + bias.w));
        *(float4*)(sH2 + (size_t)(((n4 - q * VP_QW) >> 2) * 16 + j) * 4) = v;
        if (r0 + j < row_hi) *(float4*)(H2 + (size_t)(r0 + j) * VP_H + n4) = v;
    }
    __syncthreads();
    PN_STAMP(3);
    {   // output layer: this quarter's K-slice of all 126 (128) columns
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        panel_mma<PnF32, 1, 1, 4, PnOrder::LdsTilePin>(sH2, {0}, rg3, VP_QW / 16, &acc, lane);
        const int n4 = wave * 16 + 4 * g, row = r0 + j;              // ODIM = 126: rows are 8-byte aligned -> two float2 stores
        if (row < row_hi) {
            float* dst = Opart + (size_t)q * part_stride + (size_t)row * ODIM + n4;
            const float b0 = q == 0 ? bias3[0] : 0.f, b1 = q == 0 ? bias3[1] : 0.f;
            *(float2*)dst = make_float2(acc[0] + b0, acc[1] + b1);
            if (n4 + 2 < ODIM) {
                const float b2 = q == 0 ? bias3[2] : 0.f, b3 = q == 0 ? bias3[3] : 0.f;
                *(float2*)(dst + 2) = make_float2(acc[2] + b2, acc[3] + b3);
            }
        }
    }
    PN_STAMP(4);
}

// O = ((p0 + p1) + (p2 + p3)) -- the one summation order every consumer of the partial outputs uses
__device__ __forceinline__ float vp_sum_parts(const float* __restrict__ part, size_t part_stride, size_t e) {
    return (part[e] + part[part_stride + e]) + (part[2 * part_stride + e] + part[3 * part_stride + e]);
}
__global__ void vposer_sum_parts_kernel(const float* __restrict__ part, size_t part_stride, size_t e0, size_t n, float* __restrict__ O) {
    const size_t e = e0 + (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < e0 + n) O[e] = vp_sum_parts(part, part_stride, e);
}

// dO [*, 126] -> dZpart [4][part_stride] ([*, 32] row-major): partial latent gradients of rows [row_lo, row_hi).
__global__ __launch_bounds__(512) void vposer_bwd_fused_kernel(VPoserPanels P, const float* __restrict__ dO, int row_lo, int row_hi,
                                                               const float* __restrict__ H1, const float* __restrict__ H2,
                                                               float* __restrict__ dZpart, size_t part_stride, ScaleTail tail) {
    // (tail.block == 0: one extra workgroup, FIRST in the grid -- these kernels keep one workgroup per CU (LDS), a 261st at the
    //  end would wait for a CU to come free and then run alone; first, it is done in a microsecond and hands its CU to the rest)
    // (a batch of clips: tail.nclip such workgroups, one per clip -- ScaleTail::nclip)
    if (tail.block >= 0 && (int)blockIdx.x - tail.block < tail.nclip) { scale_tail_block(scale_tail_clip(tail, (int)blockIdx.x - tail.block)); return; }
    const unsigned bid = blockIdx.x - (tail.block == 0 ? (unsigned)tail.nclip : 0u);
    __shared__ __attribute__((aligned(16))) float lds[VP_QW * 16 + VP_QW * 16 + VP_H * 16 + 8 * 256];
    float* const sdO = lds;                       // K = 126 padded to 128
    float* const sdH2 = sdO + VP_QW * 16;         // this quarter's 128 columns of dH2
    float* const sdH1 = sdH2 + VP_QW * 16;        // partial dH1 (all 512 columns)
    float* const sred = sdH1 + VP_H * 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const int q = bid & 3, r0 = row_lo + (int)(bid >> 2) * 16;
    PnRing<PnF32, 4, 4> rgB;
    PnRing<PnF32, 1, 4> rgC;
    // the masking activations before the first barrier (see vposer_bwd_split3_kernel)
    const size_t hrow = (size_t)min(r0 + j, row_hi - 1) * VP_H;
    const float4 hm2 = *(const float4*)(H2 + hrow + (q * 8 + wave) * 16 + 4 * g);
    float4 hm1[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) hm1[t] = *(const float4*)(H1 + hrow + (wave + 8 * t) * 16 + 4 * g);
    {   // dH2[:, quarter] = (dO x W3[:, quarter]) * mask(H2)
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        const int tile = q * 8 + wave;
        const float4* bf = P.w3t.f + (size_t)tile * P.w3t.nss * 64;
        PnRing<PnF32, 1, 4> rgA;
        panel_prefetch<PnF32, 1, 4>(rgA, {bf}, 8, lane);
        panel_stage<512>(sdO, dO, ODIM, r0, row_hi, 0, ODIM, 128, tid);
        __syncthreads();
        panel_mma<PnF32, 1, 1, 4, PnOrder::LdsTilePin>(sdO, {0}, rgA, 8, &acc, lane);
        {
            const float4* bfb[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) bfb[t] = P.w2t.f + ((size_t)(wave + 8 * t) * P.w2t.nss + q * (VP_QW / 16)) * 64;
            panel_prefetch<PnF32, 4, 4>(rgB, bfb, VP_QW / 16, lane);
        }
        const int n4 = tile * 16 + 4 * g;
        const float4 h = hm2;
        *(float4*)(sdH2 + (size_t)(((n4 - q * VP_QW) >> 2) * 16 + j) * 4) =
            make_float4(acc[0] * (h.x > 0.f ? 1.f : 0.2f), acc[1] * (h.y > 0.f ? 1.f : 0.2f), acc[2] * (h.z > 0.f ? 1.f : 0.2f),
                        acc[3] * (h.w > 0.f ? 1.f : 0.2f));
    }
    __syncthreads();
    {   // partial dH1 = (dH2[:, quarter] x W2[quarter rows, :]) * mask(H1): tiles wave, wave + 8, wave + 16, wave + 24
        f32x4_t acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        panel_mma<PnF32, 1, 4, 4, PnOrder::LdsTilePin>(sdH2, {0}, rgB, VP_QW / 16, acc, lane);
        {
            const float4* bfc = P.w1t.f + ((size_t)(wave & 1) * P.w1t.nss + (wave >> 1) * 8) * 64;
            panel_prefetch<PnF32, 1, 4>(rgC, {bfc}, 8, lane);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n4 = (wave + 8 * t) * 16 + 4 * g;
            const float4 h = hm1[t];
            *(float4*)(sdH1 + (size_t)((n4 >> 2) * 16 + j) * 4) =
                make_float4(acc[t][0] * (h.x > 0.f ? 1.f : 0.2f), acc[t][1] * (h.y > 0.f ? 1.f : 0.2f),
                            acc[t][2] * (h.z > 0.f ? 1.f : 0.2f), acc[t][3] * (h.w > 0.f ? 1.f : 0.2f));
        }
    }
    __syncthreads();
    {   // partial d latent = partial dH1 x W1: 2 column tiles x 4 K-slices over the 8 waves, slices summed in order
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        const int tile = wave & 1, ks = wave >> 1;
        panel_mma<PnF32, 1, 1, 4, PnOrder::LdsTilePin>(sdH1 + (size_t)ks * 8 * 256, {0}, rgC, 8, &acc, lane);
        *(float4*)(sred + (size_t)(ks * 2 + tile) * 256 + lane * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
    __syncthreads();
    if (wave < 2) {
        const float4 s0 = *(const float4*)(sred + (size_t)(0 + wave) * 256 + lane * 4), s1 = *(const float4*)(sred + (size_t)(2 + wave) * 256 + lane * 4);
        const float4 s2 = *(const float4*)(sred + (size_t)(4 + wave) * 256 + lane * 4), s3 = *(const float4*)(sred + (size_t)(6 + wave) * 256 + lane * 4);
        const int n4 = wave * 16 + 4 * g, row = r0 + j;
        if (row < row_hi)
            *(float4*)(dZpart + (size_t)q * part_stride + (size_t)row * VP_Z + n4) =
                make_float4(((s0.x + s1.x) + s2.x) + s3.x, ((s0.y + s1.y) + s2.y) + s3.y, ((s0.z + s1.z) + s2.z) + s3.z, ((s0.w + s1.w) + s2.w) + s3.w);
    }
}

__global__ void vposer_fold_dz_kernel(const float* __restrict__ part, size_t part_stride, int row_lo, int nrows, float* __restrict__ dX) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nrows * VP_Z) return;
    const int row = row_lo + e / VP_Z, c = e % VP_Z;
    dX[(size_t)row * XDIM + X_LATENT + c] += vp_sum_dz(part, part_stride, (size_t)row * VP_Z + c);
}

// ---------------------------------------------------------------------------------------------------------------------
// The fused VPoser kernels on the split format VpF (= PnF) (same decomposition: 16 rows x one quarter of the hidden columns
// per workgroup, four partial outputs / four partial latent gradients; see vposer_fwd_fused_kernel / vposer_bwd_fused_kernel).
struct VPoserPanels3 {
    PanelB3 w1, w2, w3, w3t, w2t, w1t;
    const float *b1 = nullptr, *b2 = nullptr, *b3 = nullptr;
    // what bounds a hidden row from the row before it -- |x W + b| <= c max|x| + bmax with c = the largest column 1-norm of W --
    // so every row's power-of-two scale follows from its latent's (its output gradient's) largest entry without a reduction
    float c1 = 0.f, b1max = 0.f, c2 = 0.f, b2max = 0.f, c3t = 0.f, c2t = 0.f;
};
typedef PnF VpF;                                  // operand format of the fused VPoser kernels
constexpr int VP3_PZ = (VP_Z / 8) * 16, VP3_PH = (VP_H / 8) * 16, VP3_PQ = (VP_QW / 8) * 16;     // plane strides (uint4)
// What the backward needs of the hidden activations is their SIGNS (LeakyReLU's slope): the split kernels keep one byte per four
// columns in H1 / H2 -- bit e = column 4 b + e is positive -- 128 bytes per row instead of 2 KB (late r4: what a kernel leaves dirty in
// L2 is written back when it ends, ~0.2 us per MB, tools/launch_overhead_probe.hip; the forward wrote 4 MB of activations per launch
// and the four quarter-workgroups of a row block read H1 four times over).  Indexed by absolute row: the forward's and the backward's
// 16-row blocks need not coincide (sharded runs).  The exact-fp32 twins keep floats in the same buffers.
constexpr int VP3_MROW = VP_H / 4;
#ifndef FDC_VP3_PF2
#define FDC_VP3_PF2 4
#endif
constexpr int VP3_PF2 = FDC_VP3_PF2;          // fragments of layer 2's stream in flight per wave (16 steps; the ring turns every 2 PF)
__device__ __forceinline__ unsigned char vp3_signs(const float4 v) {
    return (unsigned char)((v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u));
}

__global__ __launch_bounds__(512) void vposer_fwd_split3_kernel(VPoserPanels3 P, const float* __restrict__ Z, int ldx, int row_lo,
                                                                int row_hi, float* __restrict__ H1, float* __restrict__ H2,
                                                                float* __restrict__ Opart, size_t part_stride, VpRows two, DeferredStep ds) {
    constexpr int NP = VpF::NP;
    __shared__ __attribute__((aligned(16))) uint4 lds3[NP * (VP3_PZ + VP3_PH + VP3_PQ) + VpF::SC_U4];
    uint4* const sZ = lds3;                                      // (PnH2: the latent rows' inverse scales right behind its planes)
    uint4* const sH1 = sZ + NP * VP3_PZ + VpF::SC_U4;
    uint4* const sH2 = sH1 + NP * VP3_PH;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    int rblk = (int)(blockIdx.x >> 2);
    if (rblk >= two.nb1) { rblk -= two.nb1; row_lo = two.row2_lo; row_hi = two.row2_hi; }
    const int q = blockIdx.x & 3, r0 = row_lo + rblk * 16;
    PnRing<VpF, 1, VP3_PF2> rg2;
    PnRing<VpF, 1, 2> rg3;
    // the biases (and column scales) of all three layers, requested before the first barrier (the compiler does not move a load across
    // one): fetched where they are used -- after each layer's products -- every tile's bias was a round trip of its own
    float4 bias1[4];
    f32x4_t cs1[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { bias1[t] = *(const float4*)(P.b1 + (wave * 4 + t) * 16 + 4 * g); cs1[t] = VpF::tile_isc(P.w1, wave * 4 + t, g); }
    const float4 bias2 = *(const float4*)(P.b2 + (q * 8 + wave) * 16 + 4 * g);
    const f32x4_t cs2 = VpF::tile_isc(P.w2, q * 8 + wave, g), cs3 = VpF::tile_isc(P.w3, wave, g);
    float bias3[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) bias3[e] = P.b3[min(wave * 16 + 4 * g + e, ODIM - 1)];
    float bnd1, s1, is1;
    {   // layer 1, all 512 columns (four tiles per wave), K = 32 = one step
        VpF::Acc acc[4];
        const uint4* bf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { acc[t] = VpF::zero(); bf[t] = P.w1.f + (size_t)(wave * 4 + t) * P.w1.nst * NP * 64; }
        PnRing<VpF, 4, 1> rg1;
        panel_prefetch<VpF, 4, 1>(rg1, bf, 1, lane);
        if (ds.on)                                         // (wave-uniform) the latent rows after the pending optimiser step, straight into the image
            pnf_put_latent(sZ, VP3_PZ, tid >> 5, tid & 31, vp_deferred_latent(ds, r0, row_hi, tid));
        else
            VpF::stage<512, 1, 1>(sZ, 0, Z, ldx, r0, row_hi, 0, VP_Z, VP_Z, tid);
        __syncthreads();
        panel_mma<VpF, 1, 4, 1, PnOrder::LdsTilePin>(sZ, {VP3_PZ, 0}, rg1, 1, acc, lane);
        {
            const uint4* bf2 = P.w2.f + (size_t)(q * 8 + wave) * P.w2.nst * NP * 64;
            panel_prefetch<VpF, 1, VP3_PF2>(rg2, {bf2}, VP_H / 32, lane);
        }
        const float zis = VpF::row_isc(sZ, VP3_PZ, j);
        bnd1 = P.c1 * (16384.f * zis) + P.b1max;           // >= every |H1| of row j (2^14 zis >= its largest |z|)
        VpF::pow2(bnd1, s1, is1);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n4 = (wave * 4 + t) * 16 + 4 * g;
            const float4 bias = bias1[t];
            const f32x4_t o = VpF::value(acc[t], zis, cs1[t]);
            const float4 v = make_float4(vp_lrelu(o[0] + bias.x), vp_lrelu(o[1] + bias.y), vp_lrelu(o[2] + bias.z), vp_lrelu(o[3] + bias.w));
            pnf_lds_store4(sH1, VP3_PH, n4, j, v, s1);
            if ((n4 / VP_QW) == q && r0 + j < row_hi) ((unsigned char*)H1)[(size_t)(r0 + j) * VP3_MROW + (n4 >> 2)] = vp3_signs(v);
        }
    }
    __syncthreads();
    float s2, is2;
    {   // layer 2, this quarter's 128 columns (one tile per wave), K = 512 = 16 steps
        VpF::Acc acc = VpF::zero();
        const int tile = q * 8 + wave;
        panel_mma<VpF, 1, 1, VP3_PF2, PnOrder::LdsTilePin>(sH1, {VP3_PH, 0}, rg2, VP_H / 32, &acc, lane);
        {
            const uint4* bf3 = P.w3.f + ((size_t)wave * P.w3.nst + q * (VP_QW / 32)) * NP * 64;
            panel_prefetch<VpF, 1, 2>(rg3, {bf3}, VP_QW / 32, lane);
        }
        VpF::pow2(P.c2 * bnd1 + P.b2max, s2, is2);
        const int n4 = tile * 16 + 4 * g;
        const float4 bias = bias2;
        const f32x4_t o = VpF::value(acc, is1, cs2);
        const float4 v = make_float4(vp_lrelu(o[0] + bias.x), vp_lrelu(o[1] + bias.y), vp_lrelu(o[2] + bias.z), vp_lrelu(o[3] + bias.w));
        pnf_lds_store4(sH2, VP3_PQ, n4 - q * VP_QW, j, v, s2);
        if (r0 + j < row_hi) ((unsigned char*)H2)[(size_t)(r0 + j) * VP3_MROW + (n4 >> 2)] = vp3_signs(v);
    }
    __syncthreads();
    {   // output layer: this quarter's K-slice (128 = 4 steps) of all 126 (128) columns
        VpF::Acc acc = VpF::zero();
        panel_mma<VpF, 1, 1, 2, PnOrder::LdsTilePin>(sH2, {VP3_PQ, 0}, rg3, VP_QW / 32, &acc, lane);
        const f32x4_t o = VpF::value(acc, is2, cs3);
        const int n4 = wave * 16 + 4 * g, row = r0 + j;
        if (row < row_hi) {
            float* dst = Opart + (size_t)q * part_stride + (size_t)row * ODIM + n4;
            const float b0 = q == 0 ? bias3[0] : 0.f, b1 = q == 0 ? bias3[1] : 0.f;
            *(float2*)dst = make_float2(o[0] + b0, o[1] + b1);
            if (n4 + 2 < ODIM) {
                const float b2 = q == 0 ? bias3[2] : 0.f, b3 = q == 0 ? bias3[3] : 0.f;
                *(float2*)(dst + 2) = make_float2(o[2] + b2, o[3] + b3);
            }
        }
    }
}

__global__ __launch_bounds__(512) void vposer_bwd_split3_kernel(VPoserPanels3 P, const float* __restrict__ dO, int row_lo, int row_hi,
                                                                const float* __restrict__ H1, const float* __restrict__ H2,
                                                                float* __restrict__ dZpart, size_t part_stride, ScaleTail tail) {
    // (tail.block == 0: one extra workgroup, FIRST in the grid -- these kernels keep one workgroup per CU (LDS), a 261st at the
    //  end would wait for a CU to come free and then run alone; first, it is done in a microsecond and hands its CU to the rest)
    // (a batch of clips: tail.nclip such workgroups, one per clip -- ScaleTail::nclip)
    if (tail.block >= 0 && (int)blockIdx.x - tail.block < tail.nclip) {
        ScaleTail t2 = scale_tail_clip(tail, (int)blockIdx.x - tail.block);
        if (tail.lg_spread) t2.lg.rows = nullptr;            // (the logged sums: regular workgroups, below)
        scale_tail_block(t2);
        return;
    }
    const unsigned bid = blockIdx.x - (tail.block == 0 ? (unsigned)tail.nclip : 0u);
    constexpr int NP = VpF::NP;
    __shared__ __attribute__((aligned(16))) uint4 lds3[NP * (VP3_PQ + VP3_PQ + VP3_PH) + VpF::SC_U4 + 8 * 64];
    uint4* const sdO = lds3;                      // K = 126 padded to 128 (PnH2: + the rows' inverse scales behind the planes)
    uint4* const sdH2 = sdO + NP * VP3_PQ + VpF::SC_U4;   // this quarter's 128 columns of dH2
    uint4* const sdH1 = sdH2 + NP * VP3_PQ;       // partial dH1 (all 512 columns)
    float* const sred = (float*)(sdH1 + NP * VP3_PH);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const int q = bid & 3, r0 = row_lo + (int)(bid >> 2) * 16;
    PnRing<VpF, 4, 2> rgB;
    PnRing<VpF, 1, 2> rgC;
    // the forward activations whose signs mask this wave's tiles, requested before the first barrier (rows clamped:
    // unconditional loads).  Fetched after each layer's products they were five dependent round trips on cold data.
    const size_t hrow = (size_t)min(r0 + j, row_hi - 1) * VP3_MROW;          // (sign bytes: vp3_signs)
    const unsigned hm2 = ((const unsigned char*)H2)[hrow + (q * 8 + wave) * 4 + g];
    unsigned hm1[4];
    f32x4_t csB[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { hm1[t] = ((const unsigned char*)H1)[hrow + (wave + 8 * t) * 4 + g]; csB[t] = VpF::tile_isc(P.w2t, wave + 8 * t, g); }
    const f32x4_t csA = VpF::tile_isc(P.w3t, q * 8 + wave, g), csC = VpF::tile_isc(P.w1t, wave & 1, g);
    float bd2, sd2, isd2;
    {   // dH2[:, quarter] = (dO x W3[:, quarter]) * mask(H2)
        VpF::Acc acc = VpF::zero();
        const int tile = q * 8 + wave;
        const uint4* bf = P.w3t.f + (size_t)tile * P.w3t.nst * NP * 64;
        PnRing<VpF, 1, 2> rgA;
        panel_prefetch<VpF, 1, 2>(rgA, {bf}, 4, lane);
        if (tail.lg_spread && bid < (unsigned)LROW && wave == 0)     // (wave-uniform) one logged term: ScaleTail::lg_spread
            loss_rows_reduce_slot(tail.lg.rows, tail.row0, tail.lg.n, tail.lg.mask, tail.lg.assign, tail.lg.losses, (int)bid, lane);
        VpF::stage<512, 1, 1>(sdO, 0, dO, ODIM, r0, row_hi, 0, ODIM, 128, tid);
        __syncthreads();
        panel_mma<VpF, 1, 1, 2, PnOrder::LdsTilePin>(sdO, {VP3_PQ, 0}, rgA, 4, &acc, lane);
        {
            const uint4* bfb[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) bfb[t] = P.w2t.f + ((size_t)(wave + 8 * t) * P.w2t.nst + q * (VP_QW / 32)) * NP * 64;
            panel_prefetch<VpF, 4, 2>(rgB, bfb, VP_QW / 32, lane);
        }
        const float dois = VpF::row_isc(sdO, VP3_PQ, j);
        bd2 = P.c3t * (16384.f * dois);                   // >= every |dH2| of row j
        VpF::pow2(bd2, sd2, isd2);
        const f32x4_t o = VpF::value(acc, dois, csA);
        const int n4 = tile * 16 + 4 * g;
        const unsigned h = hm2;
        pnf_lds_store4(sdH2, VP3_PQ, n4 - q * VP_QW, j,
                       make_float4(o[0] * ((h & 1u) ? 1.f : 0.2f), o[1] * ((h & 2u) ? 1.f : 0.2f), o[2] * ((h & 4u) ? 1.f : 0.2f),
                                   o[3] * ((h & 8u) ? 1.f : 0.2f)), sd2);
    }
    __syncthreads();
    float sd1, isd1;
    {   // partial dH1 = (dH2[:, quarter] x W2[quarter rows, :]) * mask(H1): tiles wave, wave + 8, wave + 16, wave + 24
        VpF::Acc acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = VpF::zero();
        panel_mma<VpF, 1, 4, 2, PnOrder::LdsTilePin>(sdH2, {VP3_PQ, 0}, rgB, VP_QW / 32, acc, lane);
        {
            const uint4* bfc = P.w1t.f + ((size_t)(wave & 1) * P.w1t.nst + (wave >> 1) * 4) * NP * 64;
            panel_prefetch<VpF, 1, 2>(rgC, {bfc}, 4, lane);
        }
        VpF::pow2(P.c2t * bd2, sd1, isd1);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n4 = (wave + 8 * t) * 16 + 4 * g;
            const unsigned h = hm1[t];
            const f32x4_t o = VpF::value(acc[t], isd2, csB[t]);
            pnf_lds_store4(sdH1, VP3_PH, n4, j,
                           make_float4(o[0] * ((h & 1u) ? 1.f : 0.2f), o[1] * ((h & 2u) ? 1.f : 0.2f),
                                       o[2] * ((h & 4u) ? 1.f : 0.2f), o[3] * ((h & 8u) ? 1.f : 0.2f)), sd1);
        }
    }
    __syncthreads();
    {   // partial d latent = partial dH1 x W1: 2 column tiles x 4 K-slices (128 columns = 4 steps each), slices summed in order
        VpF::Acc acc = VpF::zero();
        const int tile = wave & 1, ks = wave >> 1;
        panel_mma<VpF, 1, 1, 2, PnOrder::LdsTilePin>(sdH1 + (size_t)ks * 4 * 64, {VP3_PH, 0}, rgC, 4, &acc, lane);
        const f32x4_t o = VpF::value(acc, isd1, csC);
        *(float4*)(sred + (size_t)(ks * 2 + tile) * 256 + lane * 4) = make_float4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();
    if (wave < 2) {
        const float4 s0 = *(const float4*)(sred + (size_t)(0 + wave) * 256 + lane * 4), s1 = *(const float4*)(sred + (size_t)(2 + wave) * 256 + lane * 4);
        const float4 s2 = *(const float4*)(sred + (size_t)(4 + wave) * 256 + lane * 4), s3 = *(const float4*)(sred + (size_t)(6 + wave) * 256 + lane * 4);
        const int n4 = wave * 16 + 4 * g, row = r0 + j;
        if (row < row_hi)
            *(float4*)(dZpart + (size_t)q * part_stride + (size_t)row * VP_Z + n4) =
                make_float4(((s0.x + s1.x) + s2.x) + s3.x, ((s0.y + s1.y) + s2.y) + s3.y, ((s0.z + s1.z) + s2.z) + s3.z, ((s0.w + s1.w) + s2.w) + s3.w);
    }
}

}  // namespace fdc
