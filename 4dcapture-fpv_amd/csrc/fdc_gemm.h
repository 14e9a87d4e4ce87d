// C[M,N] = A[M,K] x B^T in exact fp32 on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32: bitwise an fmaf
// chain); A [M,K] and B [N,K] row-major with leading dimensions lda / ldb, K of any length.
//
// ONE product of the library lands here: the data gradient of the pose / shape blend, dPF[F,496] = dv_off[F,3V'] x blend^T, with
// FDCAP_GEMM_SPLIT3=0 on a vertex set of more than 2048 vertices (3 V' > PANEL_MAX_K: no fp32 panel of the operand is kept -- see
// blend_backward, fdc_state.h).  Every other dense product runs on the panels of fdc_panel.h.
//
// A workgroup is four waves and owns one output tile.  The waves split each K slab between them (intra-workgroup split-K) and their
// partial tiles are summed in a fixed order through LDS, so results are reproducible; the next slab's global loads are in flight
// while the current one is multiplied.  Two tile sizes, each with scalar and with float4 staging; gemm_f32_nt chooses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdc_math.h"

namespace fdc {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// 32x32 output tile, K in slabs of 128: wave w multiplies columns [32 w, 32 w + 32) of every slab.  Operand rows are padded by one
// float in LDS so both fragment reads (lanes walk rows, fixed k) are bank-conflict free.
__global__ __launch_bounds__(256) void gemm_f32_mfma_ksplit_kernel(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, float* __restrict__ C,
    int ldc, int M, int N, int K) {
    constexpr int BM = 32, BN = 32, BK = 128, LD = BK + 1, NLD = (BM * BK) / 256;   // 16 loads per operand per thread
    __shared__ float As[BM * LD];
    __shared__ float Bs[BN * LD];
    __shared__ float Red[3][BM * BN];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float ra[NLD], rb[NLD];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            int e = tid + i * 256, r = e >> 7, c = e & 127;
            int gm = m0 + r, gk = k0 + c;
            ra[i] = (gm < M && gk < K) ? A[(size_t)gm * lda + gk] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            int e = tid + i * 256, r = e >> 7, c = e & 127;
            int gn = n0 + r, gk = k0 + c;
            rb[i] = (gn < N && gk < K) ? B[(size_t)gn * ldb + gk] : 0.f;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            int e = tid + i * 256;
            As[(e >> 7) * LD + (e & 127)] = ra[i];
            Bs[(e >> 7) * LD + (e & 127)] = rb[i];
        }
    };
    gload(0);
    for (int k0 = 0; k0 < K; k0 += BK) {
        lstore();
        __syncthreads();
        if (k0 + BK < K) gload(k0 + BK);                    // in flight during the MFMAs below
        const int kq = wave * 32;                           // this wave's quarter of the slab
#pragma unroll 4
        for (int kk = 0; kk < 32; kk += 2) {
            float a = As[(lane & 31) * LD + kq + kk + (lane >> 5)];
            float b = Bs[(lane & 31) * LD + kq + kk + (lane >> 5)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // fixed-order reduction of the four K-quarters: ((w0 + w1) + w2) + w3
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) Red[wave - 1][r * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = acc[r] + Red[0][r * 64 + lane];
            v += Red[1][r * 64 + lane];
            v += Red[2][r * 64 + lane];
            // C/D layout of the 32x32 tile: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
            int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            int n = n0 + (lane & 31);
            if (m < M && n < N) C[(size_t)m * ldc + n] = v;
        }
    }
}

// Vectorised staging for the 32x32 tile: 16-byte global loads and ds_write_b128 / ds_read_b128 instead of one dword per
// instruction -- a quarter of the vector-memory and LDS instructions per slab (a timing ablation of the scalar kernel put ~1/3 of
// its time in the load + LDS-store phase, none in the fragment reads).  Needs 16-byte aligned operand rows (lda, ldb and K
// multiples of 4, aligned bases); gemm_f32_nt falls back to the scalar kernel otherwise.  K order inside a wave's 32-deep quarter
// is permuted so that one float4 feeds four MFMAs: MFMA j of group q multiplies k = 8q + j (lanes 0-31) and k = 8q + 4 + j
// (lanes 32-63) -- any pairing is valid as long as A and B use the same one; the sum over k is the same set of products.
__global__ __launch_bounds__(256) void gemm_f32_mfma_ksplit_v4_kernel(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, float* __restrict__ C,
    int ldc, int M, int N, int K) {
    constexpr int BM = 32, BN = 32, BK = 128, LD = BK + 4, NV = (BM * BK) / (4 * 256);   // 4 float4 per operand per thread
    __shared__ __attribute__((aligned(16))) float As[BM * LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN * LD];
    __shared__ float Red[3][BM * BN];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, col = lane & 31;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ra[NV], rb[NV];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * 256, r = e >> 5, c4 = e & 31;
            const int gm = m0 + r, gk = k0 + 4 * c4;
            ra[i] = z4;
            if (gm < M && gk < K) ra[i] = *reinterpret_cast<const float4*>(A + (size_t)gm * lda + gk);
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * 256, r = e >> 5, c4 = e & 31;
            const int gn = n0 + r, gk = k0 + 4 * c4;
            rb[i] = z4;
            if (gn < N && gk < K) rb[i] = *reinterpret_cast<const float4*>(B + (size_t)gn * ldb + gk);
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * 256;
            *reinterpret_cast<float4*>(&As[(e >> 5) * LD + 4 * (e & 31)]) = ra[i];
            *reinterpret_cast<float4*>(&Bs[(e >> 5) * LD + 4 * (e & 31)]) = rb[i];
        }
    };
    gload(0);
    for (int k0 = 0; k0 < K; k0 += BK) {
        lstore();
        __syncthreads();
        if (k0 + BK < K) gload(k0 + BK);                    // in flight during the MFMAs below
        const int kq = wave * 32;                           // this wave's quarter of the slab
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int kb = kq + 8 * q + 4 * half;
            const float4 a4 = *reinterpret_cast<const float4*>(&As[col * LD + kb]);
            const float4 b4 = *reinterpret_cast<const float4*>(&Bs[col * LD + kb]);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // fixed-order reduction of the four K-quarters: ((w0 + w1) + w2) + w3
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) Red[wave - 1][r * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = acc[r] + Red[0][r * 64 + lane];
            v += Red[1][r * 64 + lane];
            v += Red[2][r * 64 + lane];
            int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            int n = n0 + col;
            if (m < M && n < N) C[(size_t)m * ldc + n] = v;
        }
    }
}

// The same scheme on 16x16 output tiles (v_mfma_f32_16x16x4_f32): four times the workgroups and a 19 KB LDS footprint, for
// products whose 32x32 grid leaves most CUs with one or two workgroups -- there every K slab costs a full, exposed global-load
// latency (one slab = 2 x TS x 128 floats in flight per workgroup), and only more resident workgroups per CU hide it.  Same
// fixed-order sum of the four K-quarters.
__global__ __launch_bounds__(256) void gemm_f32_mfma_ksplit16_kernel(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, float* __restrict__ C,
    int ldc, int M, int N, int K) {
    constexpr int TS = 16, BK = 128, LD = BK + 1, NLD = (TS * BK) / 256;   // 8 loads per operand per thread
    __shared__ float As[TS * LD];
    __shared__ float Bs[TS * LD];
    __shared__ float Red[3][TS * TS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m0 = blockIdx.y * TS, n0 = blockIdx.x * TS;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    float ra[NLD], rb[NLD];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            int e = tid + i * 256, r = e >> 7, c = e & 127;
            int gm = m0 + r, gk = k0 + c;
            ra[i] = (gm < M && gk < K) ? A[(size_t)gm * lda + gk] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            int e = tid + i * 256, r = e >> 7, c = e & 127;
            int gn = n0 + r, gk = k0 + c;
            rb[i] = (gn < N && gk < K) ? B[(size_t)gn * ldb + gk] : 0.f;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            int e = tid + i * 256;
            As[(e >> 7) * LD + (e & 127)] = ra[i];
            Bs[(e >> 7) * LD + (e & 127)] = rb[i];
        }
    };
    gload(0);
    for (int k0 = 0; k0 < K; k0 += BK) {
        lstore();
        __syncthreads();
        if (k0 + BK < K) gload(k0 + BK);                    // in flight during the MFMAs below
        const int kq = wave * 32;                           // this wave's quarter of the slab
#pragma unroll
        for (int kk = 0; kk < 32; kk += 4) {
            float a = As[(lane & 15) * LD + kq + kk + (lane >> 4)];
            float b = Bs[(lane & 15) * LD + kq + kk + (lane >> 4)];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Red[wave - 1][r * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = acc[r] + Red[0][r * 64 + lane];
            v += Red[1][r * 64 + lane];
            v += Red[2][r * 64 + lane];
            int m = m0 + 4 * (lane >> 4) + r;               // C/D layout of the 16x16 tile: col = lane & 15, row = 4 * (lane >> 4) + reg
            int n = n0 + (lane & 15);
            if (m < M && n < N) C[(size_t)m * ldc + n] = v;
        }
    }
}

// 16x16 tiles with the vectorised staging of gemm_f32_mfma_ksplit_v4_kernel, K in slabs of 256 (deep products on small grids: half
// the slab rounds -- barriers + exposed load latencies).  v_mfma_f32_16x16x4_f32: lane group g = lane >> 4 supplies k = 4 s + g of
// step s; with one float4 per lane, MFMA j of group q multiplies k = 16 q + 4 g + j.
__global__ __launch_bounds__(256) void gemm_f32_mfma_ksplit16_v4_kernel(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, float* __restrict__ C,
    int ldc, int M, int N, int K) {
    constexpr int TS = 16, BK = 256, LD = BK + 4, NV = (TS * BK) / (4 * 256), C4 = BK / 4, KW = BK / 4;   // NV float4 per operand per thread; C4 float4 per row; KW k per wave and slab
    __shared__ __attribute__((aligned(16))) float As[TS * LD];
    __shared__ __attribute__((aligned(16))) float Bs[TS * LD];
    __shared__ float Red[3][TS * TS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, grp = lane >> 4, col = lane & 15;
    const int m0 = blockIdx.y * TS, n0 = blockIdx.x * TS;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ra[NV], rb[NV];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * 256, r = e / C4, c4 = e % C4;
            const int gm = m0 + r, gk = k0 + 4 * c4;
            ra[i] = z4;
            if (gm < M && gk < K) ra[i] = *reinterpret_cast<const float4*>(A + (size_t)gm * lda + gk);
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * 256, r = e / C4, c4 = e % C4;
            const int gn = n0 + r, gk = k0 + 4 * c4;
            rb[i] = z4;
            if (gn < N && gk < K) rb[i] = *reinterpret_cast<const float4*>(B + (size_t)gn * ldb + gk);
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * 256;
            *reinterpret_cast<float4*>(&As[(e / C4) * LD + 4 * (e % C4)]) = ra[i];
            *reinterpret_cast<float4*>(&Bs[(e / C4) * LD + 4 * (e % C4)]) = rb[i];
        }
    };
    gload(0);
    for (int k0 = 0; k0 < K; k0 += BK) {
        lstore();
        __syncthreads();
        if (k0 + BK < K) gload(k0 + BK);                    // in flight during the MFMAs below
        const int kq = wave * KW;                           // this wave's quarter of the slab
#pragma unroll
        for (int q = 0; q < KW / 16; ++q) {
            const int kb = kq + 16 * q + 4 * grp;
            const float4 a4 = *reinterpret_cast<const float4*>(&As[col * LD + kb]);
            const float4 b4 = *reinterpret_cast<const float4*>(&Bs[col * LD + kb]);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b4.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b4.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b4.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b4.w, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Red[wave - 1][r * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = acc[r] + Red[0][r * 64 + lane];
            v += Red[1][r * 64 + lane];
            v += Red[2][r * 64 + lane];
            int m = m0 + 4 * grp + r;
            int n = n0 + col;
            if (m < M && n < N) C[(size_t)m * ldc + n] = v;
        }
    }
}

// C[M,N] = A[M,K] x B^T (B stored [N,K]), exact fp32.  The caller's products are deep (K > 6144) and at most a few hundred columns
// wide; both rules below were measured on such shapes.
static inline hipError_t gemm_f32_nt(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
                                     hipStream_t st) {
    if (M <= 0 || N <= 0) return hipSuccess;
    // 16x16 tiles read twice the operand bytes per MAC: they pay off while the 32x32 grid is small (latency-bound) -- fewer than 256
    // tiles; from there on the product is L2-bandwidth-bound with them
    const long long tiles32 = (long long)((N + 31) / 32) * ((M + 31) / 32);
    // float4 staging whenever the operands allow it; the scalar-staging kernels serve the rest
    const bool aligned = (lda % 4 == 0) && (ldb % 4 == 0) && (K % 4 == 0) &&
                         ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) == 0;
    const bool t16 = tiles32 < 256;
    const dim3 grid(t16 ? (N + 15) / 16 : (N + 31) / 32, t16 ? (M + 15) / 16 : (M + 31) / 32);
    void (*kernel)(const float*, int, const float*, int, float*, int, int, int, int);
    if (t16 && aligned) { kernel = gemm_f32_mfma_ksplit16_v4_kernel; note_form("gemm_f32_mfma_ksplit16_v4_kernel"); }
    else if (t16) { kernel = gemm_f32_mfma_ksplit16_kernel; note_form("gemm_f32_mfma_ksplit16_kernel"); }
    else if (aligned) { kernel = gemm_f32_mfma_ksplit_v4_kernel; note_form("gemm_f32_mfma_ksplit_v4_kernel"); }
    else { kernel = gemm_f32_mfma_ksplit_kernel; note_form("gemm_f32_mfma_ksplit_kernel"); }
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, A, lda, B, ldb, C, ldc, M, N, K);
    return hipGetLastError();
}

}  // namespace fdc
