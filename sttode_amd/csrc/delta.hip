// Gromov delta-hyperbolicity of point sets (hyptorch/delta.py:12-35, Khrulkov et al., "Hyperbolic Image Embeddings"): include/sttode_hip.h
// sttode_delta_dist / sttode_delta_workspace / sttode_delta_hyp, DESIGN.md §4m.
//   delta_dist_kernel    T x (64 x 64)-tiles of pairwise Euclidean distances of rows of X (gathered through idx), direct-difference form
//                        sqrt(sum_k (x_i - x_j)^2) in fp32 with k in order for every pair: (i, j) and (j, i) run the same operations on the
//                        same values, so dist is bitwise symmetric with an exact zero diagonal.  The try's diameter is folded in: a
//                        workgroup maximum, then an integer atomicMax on the bits (distances are >= 0, so the bits order like the values).
//   delta_tile_kernel    the max-min ("tropical") product C = A (max.min) A of the Gromov products A = 0.5 ((D[0, j] + D[i, 0]) - D[i, j]),
//                        register-tiled like a GEMM: 128 x 128 (i, j) tiles, each lane a block of 8 x 8 running maxima, k-panels of 32 of
//                        both operands formed from D while they are staged into LDS.  The epilogue subtracts A[i, j] and writes the tile's
//                        maximum of C - A to its own workspace slot.  Neither A nor C exists as an n^2 buffer.
//   delta_reduce_kernel  one workgroup per try: the maximum over the try's tile slots.  Max is exact, so the result has no order question.
#include "api_util.hpp"
#include "../../include/sttode_hip.h"

// No contraction anywhere in this file: the Gromov product and C - A must round exactly as written (the epilogue's C - 0.5 (...) would
// otherwise become one fma), and every distance runs the same sub / mul / add sequence.
#pragma clang fp contract(off)

namespace {

constexpr int DT = 64;        // distance tile (rows x columns), 256 lanes of 4 x 4
constexpr int DK = 16;        // feature columns per LDS panel of the distance kernel
constexpr int BT = 128;       // delta tile (i x j), 256 lanes of 8 x 8
constexpr int BK = 32;        // k per LDS panel of the delta kernel
constexpr int LDA = BT + 4;   // padded LDS row of the delta kernel's panels (16-byte aligned rows)
constexpr int MAX_N = 32768;
constexpr int MAX_T = 65535;  // tries ride on gridDim.y

// Single-instruction min / max: fminf / fmaxf on values loaded from memory make the compiler canonicalise both operands first
// (v_max_f32 x, x in front of each), which would double the inner loop.  The values here are finite or -inf, never NaN.
__device__ __forceinline__ float vmin(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// Gromov product w.r.t. the base point 0, in the reference's order (delta.py:19: 0.5 * (row + col - dismat)); row + col is one fp32 add,
// commutative, so A[i, j] of a bitwise-symmetric D is bitwise symmetric.
__device__ __forceinline__ float gromov(float d0j, float di0, float dij) {
    return 0.5f * ((d0j + di0) - dij);
}

// grid (tiles of 64 x 64 per try, T), 256 lanes; lane (tx, ty) owns rows i0 + 4 ty + r, columns j0 + 4 tx + c.
__global__ __launch_bounds__(256) void delta_dist_kernel(const float* __restrict__ X, int rows, int d, const int* __restrict__ idx, int n,
                                                         float* __restrict__ dist, float* __restrict__ diam) {
    __shared__ float xi[DK][DT + 4], xj[DK][DT + 4];
    __shared__ int ri[DT], rj[DT];
    __shared__ float red[4];
    const int tn = (n + DT - 1) / DT;
    const int t = blockIdx.y;
    const int i0 = (blockIdx.x / tn) * DT, j0 = (blockIdx.x % tn) * DT;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int* ix = idx ? idx + (size_t)t * n : nullptr;
    if (tid < 2 * DT) {
        const int p = (tid < DT ? i0 : j0) + (tid & (DT - 1));
        int r = -1;
        if (p < n) {
            r = ix ? ix[p] : p;
            if (r < 0 || r >= rows) r = -2;                   // an index outside X: NaN distances, nothing read
        }
        (tid < DT ? ri : rj)[tid & (DT - 1)] = r;
    }
    __syncthreads();
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (int k0 = 0; k0 < d; k0 += DK) {
        // 2 x 64 rows x 16 columns: lane -> (row = e / 16, column = e % 16), 16 consecutive floats of a row per 16 lanes
#pragma unroll
        for (int q = 0; q < (2 * DT * DK) / 256; ++q) {
            const int e = tid + 256 * q;
            const int side = e / (DT * DK), w = e % (DT * DK), rr = w / DK, kk = w % DK;
            const int r = (side ? rj : ri)[rr];
            const int k = k0 + kk;
            float v = 0.f;                                      // padding (rows past n, columns past d) adds exact zeros
            if (r == -2) v = __builtin_nanf("");
            else if (r >= 0 && k < d) v = X[(size_t)r * d + k];
            (side ? xj : xi)[kk][rr] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < DK; ++kk) {
            const float4 a4 = *reinterpret_cast<const float4*>(&xi[kk][4 * ty]);
            const float4 b4 = *reinterpret_cast<const float4*>(&xj[kk][4 * tx]);
            const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float df = av[a] - bv[b];
                    acc[a][b] += df * df;
                }
        }
        __syncthreads();
    }
    float m = 0.f;
    bool nan = false;
    float* out = dist + (size_t)t * n * n;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + 4 * ty + a;
        if (i >= n) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + 4 * tx + b;
            if (j >= n) continue;
            const float v = sqrtf(acc[a][b]);
            out[(size_t)i * n + j] = v;
            nan |= v != v;
            m = fmaxf(m, v);
        }
    }
    m = wave_max(m);
    const bool anynan = __any(nan);
    if ((tid & 63) == 0) red[tid >> 6] = anynan ? __builtin_nanf("") : m;
    __syncthreads();
    if (tid == 0) {
        float r = red[0];
        for (int w = 1; w < 4; ++w) r = (red[w] != red[w] || r != r) ? __builtin_nanf("") : fmaxf(r, red[w]);
        atomicMax(reinterpret_cast<unsigned*>(diam) + t, __float_as_uint(r));   // NaN's bits order above every distance: NaN wins
    }
}

// grid (tiles per try, T), 256 lanes.  full: tile b -> (b / tn, b % tn); symmetric: the upper triangle bj >= bi in row order.
// Lane (tx, ty) owns rows {4 ty + r, 64 + 4 ty + r} and columns {4 tx + c, 64 + 4 tx + c} of the tile (conflict-free 16-byte LDS reads).
__global__ __launch_bounds__(256) void delta_tile_kernel(const float* __restrict__ dist, int n, int symmetric, float* __restrict__ part) {
    __shared__ float as[BK][LDA], bs[BK][LDA];
    __shared__ float coli[BT], rowj[BT];
    __shared__ float red[4];
    const int tn = (n + BT - 1) / BT;
    const int t = blockIdx.y;
    int bi, bj;
    if (symmetric) {
        int b = blockIdx.x;
        bi = 0;
        while (b >= tn - bi) {
            b -= tn - bi;
            ++bi;
        }
        bj = bi + b;
    } else {
        bi = blockIdx.x / tn;
        bj = blockIdx.x % tn;
    }
    const int i0 = bi * BT, j0 = bj * BT;
    const float* D = dist + (size_t)t * n * n;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (tid < BT) coli[tid] = i0 + tid < n ? D[(size_t)(i0 + tid) * n] : 0.f;
    else rowj[tid - BT] = j0 + tid - BT < n ? D[j0 + tid - BT] : 0.f;
    __syncthreads();
    const float NEG = -__builtin_inff();
    float acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = NEG;
    // staging roles fixed per lane: as -- column kk = tid % 32 of rows ii = tid / 32 + 8 q; bs -- column jj = tid % 128 of k rows tid / 128 + 2 q
    const int akk = tid % BK, aii = tid / BK;
    const int bjj = tid % BT, bkk = tid / BT;
    const float b_d0j = rowj[bjj];
    for (int k0 = 0; k0 < n; k0 += BK) {
        {
            const int k = k0 + akk;
            const float d0k = k < n ? D[k] : 0.f;
#pragma unroll
            for (int q = 0; q < (BT * BK) / 256; ++q) {
                const int ii = aii + 8 * q, i = i0 + ii;
                as[akk][ii] = (i < n && k < n) ? gromov(d0k, coli[ii], D[(size_t)i * n + k]) : NEG;   // A[i, k]
            }
        }
#pragma unroll
        for (int q = 0; q < (BT * BK) / 256; ++q) {
            const int kk = bkk + 2 * q, k = k0 + kk, j = j0 + bjj;
            bs[kk][bjj] = (j < n && k < n) ? gromov(b_d0j, D[(size_t)k * n], D[(size_t)k * n + j]) : NEG;   // A[k, j]
        }
        __syncthreads();
#pragma unroll 2
        for (int kk = 0; kk < BK; kk += 2) {
            float a0[8], a1[8], b0[8], b1[8];
            *reinterpret_cast<float4*>(a0) = *reinterpret_cast<const float4*>(&as[kk][4 * ty]);
            *reinterpret_cast<float4*>(a0 + 4) = *reinterpret_cast<const float4*>(&as[kk][64 + 4 * ty]);
            *reinterpret_cast<float4*>(a1) = *reinterpret_cast<const float4*>(&as[kk + 1][4 * ty]);
            *reinterpret_cast<float4*>(a1 + 4) = *reinterpret_cast<const float4*>(&as[kk + 1][64 + 4 * ty]);
            *reinterpret_cast<float4*>(b0) = *reinterpret_cast<const float4*>(&bs[kk][4 * tx]);
            *reinterpret_cast<float4*>(b0 + 4) = *reinterpret_cast<const float4*>(&bs[kk][64 + 4 * tx]);
            *reinterpret_cast<float4*>(b1) = *reinterpret_cast<const float4*>(&bs[kk + 1][4 * tx]);
            *reinterpret_cast<float4*>(b1 + 4) = *reinterpret_cast<const float4*>(&bs[kk + 1][64 + 4 * tx]);
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[a][b] = vmax3(acc[a][b], vmin(a0[a], b0[b]), vmin(a1[a], b1[b]));
        }
        __syncthreads();
    }
    float m = NEG;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const int ii = (a < 4 ? 4 * ty + a : 64 + 4 * ty + a - 4), i = i0 + ii;
        if (i >= n) continue;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int jj = (b < 4 ? 4 * tx + b : 64 + 4 * tx + b - 4), j = j0 + jj;
            if (j >= n) continue;
            m = fmaxf(m, acc[a][b] - gromov(rowj[jj], coli[ii], D[(size_t)i * n + j]));   // C[i, j] - A[i, j]
        }
    }
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) part[(size_t)t * gridDim.x + blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void delta_reduce_kernel(const float* __restrict__ part, int tiles, float* __restrict__ delta) {
    __shared__ float red[4];
    const float* p = part + (size_t)blockIdx.x * tiles;
    float m = -__builtin_inff();
    for (int b = threadIdx.x; b < tiles; b += 256) m = fmaxf(m, p[b]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) delta[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

long delta_tiles(int n, int symmetric) {
    const long tn = (n + BT - 1) / BT;
    return symmetric ? tn * (tn + 1) / 2 : tn * tn;
}

}  // namespace

extern "C" int sttode_delta_dist(const float* X, int rows, int d, const int* idx, int T, int n, float* dist, long dist_floats, float* diam,
                                 void* stream) {
    STT_REQUIRE(X && dist && diam, "sttode_delta_dist: null pointer");
    STT_REQUIRE(rows >= 1 && d >= 1, "sttode_delta_dist: X must have rows >= 1 and d >= 1");
    STT_REQUIRE(n >= 1 && n <= MAX_N, "sttode_delta_dist: n must be in [1, 32768]");
    STT_REQUIRE(T >= 1 && T <= MAX_T, "sttode_delta_dist: T must be in [1, 65535]");
    STT_REQUIRE(idx || (T == 1 && n == rows), "sttode_delta_dist: without idx, T must be 1 and n must equal rows");
    STT_REQUIRE(dist_floats >= (long)T * n * n, "sttode_delta_dist: dist holds fewer than T n^2 floats");
    hipStream_t s = (hipStream_t)stream;
    STT_HIP(hipMemsetAsync(diam, 0, sizeof(float) * T, s));
    const long tn = (n + DT - 1) / DT;
    hipLaunchKernelGGL(delta_dist_kernel, dim3((unsigned)(tn * tn), T), dim3(256), 0, s, X, rows, d, idx, n, dist, diam);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_delta_workspace(int T, int n, long* floats) {
    STT_REQUIRE(floats, "sttode_delta_workspace: null pointer");
    STT_REQUIRE(n >= 1 && n <= MAX_N, "sttode_delta_workspace: n must be in [1, 32768]");
    STT_REQUIRE(T >= 1 && T <= MAX_T, "sttode_delta_workspace: T must be in [1, 65535]");
    *floats = (long)T * delta_tiles(n, 0);
    return 0;
}

extern "C" int sttode_delta_hyp(const float* dist, int T, int n, long dist_floats, int symmetric, float* ws, long ws_floats, float* delta,
                                void* stream) {
    STT_REQUIRE(dist && ws && delta, "sttode_delta_hyp: null pointer");
    STT_REQUIRE(n >= 1 && n <= MAX_N, "sttode_delta_hyp: n must be in [1, 32768]");
    STT_REQUIRE(T >= 1 && T <= MAX_T, "sttode_delta_hyp: T must be in [1, 65535]");
    STT_REQUIRE(symmetric == 0 || symmetric == 1, "sttode_delta_hyp: symmetric must be 0 or 1");
    STT_REQUIRE(dist_floats >= (long)T * n * n, "sttode_delta_hyp: dist holds fewer than T n^2 floats");
    const long tiles = delta_tiles(n, symmetric);
    STT_REQUIRE(ws_floats >= (long)T * tiles, "sttode_delta_hyp: workspace smaller than sttode_delta_workspace says");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(delta_tile_kernel, dim3((unsigned)tiles, T), dim3(256), 0, s, dist, n, symmetric, ws);
    hipLaunchKernelGGL(delta_reduce_kernel, dim3(T), dim3(256), 0, s, (const float*)ws, (int)tiles, delta);
    STT_HIP(hipGetLastError());
    return 0;
}
