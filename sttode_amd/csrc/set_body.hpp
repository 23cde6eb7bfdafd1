// Device pieces shared by the kernels that work on sample sets (metrics.hip, weighted.hip, large_set.hip, reduce.hip, reduce_scenes.hip,
// sampler*.hip, multimodal.hip).  Each helper fixes ONE order of operations, stated on it: the promises of equal bits between
// these kernels hold because they all call the same text.  No helper knows its caller.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

#include "frontend_body.hpp"

// ---- sums and extrema over a wave / a workgroup of 256 ----------------------------------------------------------------------------------

// The 64 lanes' values by the xor tree 32, 16, ... 1: every lane gets the result, and all lanes get the same bits.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {   // (fmin: a NaN lane is skipped)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// Quads first: red[0 .. 255] holds one value per thread (the caller's barrier lies in between); lane l of ONE wave adds those of threads
// l, l + 64, l + 128, l + 192 in that order, then the 64 lanes by the xor tree.
__device__ __forceinline__ double quad_then_wave_sum(const double* red, int lane) {
    return wave_sum(((red[lane] + red[lane + 64]) + red[lane + 128]) + red[lane + 192]);
}

// Waves first: NV values per thread, each by the xor tree within its wave, then the four waves' sums in wave order; every thread gets the
// results.  red: [4][NV] of LDS.  Two barriers, the first in front of the stores (the last use of red is over).
template <int NV>
__device__ __forceinline__ void wave_then_block_sum(double (&v)[NV], double (*red)[NV]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = wave_sum(v[q]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < NV; ++q) red[w][q] = v[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
}

// Index tree: the 256 threads' values through red[256] by halving over the THREAD index (thread t adds t + 128, then t + 64, ... t + 1): a
// different order from the two above.  Every thread gets the sum.  Barriers inside, the first in front of the stores.
__device__ __forceinline__ double index_tree_block_sum(double v, double* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

// ---- (value, index) selection: by value, the LOWER index on equal values.  A NaN offered never wins; the index stays one that was offered.
template <typename T>
__device__ __forceinline__ void take_lower(T& v, int& i, T ov, int oi) {
    if (ov < v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}
template <typename T>
__device__ __forceinline__ void take_higher(T& v, int& i, T ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}
// ... over the wave by the xor tree 32 ... 1: every lane gets the same (value, index).
template <typename T>
__device__ __forceinline__ void wave_take_lower(T& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) take_lower(v, i, __shfl_xor(v, o, 64), __shfl_xor(i, o, 64));
}
template <typename T>
__device__ __forceinline__ void wave_take_higher(T& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) take_higher(v, i, __shfl_xor(v, o, 64), __shfl_xor(i, o, 64));
}

// Inclusive prefix minimum over the lanes (fminf: NaN skipped).  Lanes below 63 then take the minimum with +inf: a prefix of k < 64 values
// that are all NaN gives +inf (k = 64: NaN), as the selection of those k samples among 64 lanes whose idle ones hold +inf.
__device__ __forceinline__ float prefix_fmin64(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_up(v, o, 64);
        if (lane >= o) v = fminf(v, u);
    }
    return lane < 63 ? fminf(v, INFINITY) : v;
}

// ---- indexing ---------------------------------------------------------------------------------------------------------------------------

// Pair q of K items in F.pdist order -- (0,1), (0,2), ... (K-2,K-1) -- as (i, j), i < j.  q < K (K - 1) / 2.  pdist_row returns i and leaves in q
// the pair's place in row i: j = i + 1 + q.
__device__ __forceinline__ int pdist_row(int& q, int K) {
    int i = 0;
    while (q >= K - 1 - i) {
        q -= K - 1 - i;
        ++i;
    }
    return i;
}
__device__ __forceinline__ void pdist_pair(int q, int K, int& i, int& j) {
    i = pdist_row(q, K);
    j = i + 1 + q;
}

// Element index of sample m's row of agent a in a round-major buffer [R][n][K_in][L]: sample m = r K_in + k.
__device__ __forceinline__ size_t round_major_row(int a, int m, int n, int K_in, int L) {
    const int r = m / K_in, k = m - r * K_in;
    return (((size_t)r * n + a) * K_in + k) * (size_t)L;
}

// Segment s of a CSR as [a0, a1) clamped to [0, n] and to a0 <= a1: no address depends on seg_ptr's contents being sane.
__device__ __forceinline__ void clamped_segment(const int* __restrict__ seg_ptr, int s, int n, int& a0, int& a1) {
    a0 = min(max(seg_ptr[s], 0), n);
    a1 = min(max(seg_ptr[s + 1], a0), n);
}

// ---- frame tiles of one agent's K <= 64 samples (sample_spread_kernel, weighted_set_kernel; the constants also large_spread_kernel) -------

constexpr int SET_FT = 32;              // frames per LDS tile
constexpr int SET_STRIDE = SET_FT + 1;  // row stride in float2: odd, so that lanes on different samples at one frame fall on different banks
constexpr int SET_K1 = 23;              // the largest K with one pair per thread at most: 23 * 22 / 2 = 253 <= 256

// Frames [t0, t0 + ft) of the K samples p [K][Tf] into sx (raw float2, rows of SET_STRIDE) and of the ground truth g (may be null) into sg, by
// the workgroup's 256 threads.  The caller's barrier follows.  Row: the type the row offset k Tf is formed in (int where K Tf < 2^31 is given:
// the address arithmetic in front of the load is on the kernel's critical path).
template <typename Row>
__device__ __forceinline__ void stage_tile(float2* sx, float2* sg, const float2* __restrict__ p, const float2* __restrict__ g, int K, int Tf,
                                           int t0, int ft, int tid) {
    for (int i = tid; i < K * ft; i += 256) {
        const int k = i / ft, tl = i - k * ft;
        sx[k * SET_STRIDE + tl] = p[(Row)k * Tf + t0 + tl];
    }
    if (g && tid < ft) sg[tid] = g[t0 + tid];
}

// One pair ij = i | j << 8 over the tile's frames in frame order: coordinates (double)(x * scale) with the product in fp32, then float64:
// s2 += d^2, dl = d (the last frame's stays), s1 += d.
__device__ __forceinline__ void pair_tile_accumulate(const float2* sx, int ij, int ft, float scale, double& s2, double& s1, double& dl) {
    const float2* xi = sx + (ij & 255) * SET_STRIDE;
    const float2* xj = sx + (ij >> 8) * SET_STRIDE;
    for (int tl = 0; tl < ft; ++tl) {
        const float2 u = xi[tl], v = xj[tl];
        const double dx = (double)(u.x * scale) - (double)(v.x * scale), dy = (double)(u.y * scale) - (double)(v.y * scale);
        const double d2 = dx * dx + dy * dy;
        dl = sqrt(d2);
        s2 += d2;
        s1 += dl;
    }
}

// Sample k against the ground truth over the tile's frames in frame order: the float64 distance (ga += d, gl = d) and bok_select_kernel's
// fp32 one (bok_dist: fa += d, fl = d).
__device__ __forceinline__ void gt_tile_accumulate(const float2* sx, const float2* sg, int k, int ft, float scale, double& ga, double& gl,
                                                   float& fa, float& fl) {
    for (int tl = 0; tl < ft; ++tl) {
        const float2 v = sx[k * SET_STRIDE + tl], y = sg[tl];
        const double dx = (double)(v.x * scale) - (double)(y.x * scale), dy = (double)(v.y * scale) - (double)(y.y * scale);
        gl = sqrt(dx * dx + dy * dy);
        ga += gl;
        fl = bok_dist(v.x, v.y, y.x, y.y, scale);
        fa += fl;
    }
}

// ---- one frame of the KDE NLL (kde_nll_kernel, weighted_set_kernel, large_kde_kernel; the loops over the samples are the kernels' own) -----

// Covariance C of the frame -> det C and 1 / (f^2 det C): Sigma = f^2 C, Sigma^-1 = [[c11, -c01], [-c01, c00]] / (f^2 det C).  False where C is
// not positive definite (gaussian_kde raises there: the kernels give NaN).
__device__ __forceinline__ bool kde_cov(double c00, double c01, double c11, double f2, double& det, double& inv) {
    det = c00 * c11 - c01 * c01;
    inv = 1.0 / (f2 * det);
    return c00 > 0.0 && det > 0.0;
}
// (dx, dy)^T Sigma^-1 (dx, dy)
__device__ __forceinline__ double kde_quad(double c00, double c01, double c11, double inv, double dx, double dy) {
    return (c11 * dx * dx - 2.0 * c01 * dx * dy + c00 * dy * dy) * inv;
}
// log det(2 pi Sigma) / 2, det(2 pi Sigma) = (2 pi f^2)^2 det C
__device__ __forceinline__ double kde_log_norm(double f2, double det) {
    const double tf2 = 6.283185307179586 * f2;
    return 0.5 * log(tf2 * tf2 * det);
}
// Trajectron++'s clip of a frame's log-density
__device__ __forceinline__ double kde_clip(double lp) { return lp < -20.0 ? -20.0 : lp; }

// ---- Lloyd reductions (reduce.hip, reduce_scenes.hip; large_set.hip takes the same sets) ---------------------------------------------------

constexpr int NT = 256;                       // lanes per workgroup
constexpr int MAX_K = 64, MAX_M = 4096, MAX_TF = 200, MAX_ITERS = 1000;
constexpr int LDS_LIMIT = 159 * 1024;         // dynamic LDS of one workgroup: gfx950's 160 KiB less 1 KiB for the static words of the barrier-or

__host__ __device__ inline int up16(int b) { return (b + 15) & ~15; }

// Stable counting sort of the M samples by label lab[m] < K, by the workgroup's NT threads: per 64-sample chunk one ballot per k gives each
// sample its rank among the chunk's members of its cluster (rnk) and the chunk's member counts; wave 0 turns those into exclusive prefixes
// over the chunks (ccnt [chunks][KP]) and forms the cluster sizes cnt and offsets off.  Sample m then belongs at sorted_slot(m): the members
// of a cluster stand IN SAMPLE ORDER.  Two barriers inside, the second behind the last store.
__device__ __forceinline__ void sort_by_label(const unsigned char* lab, int M, int K, int KP, int chunks, unsigned short* rnk,
                                              unsigned short* ccnt, int* cnt, int* off) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < chunks; c += NT / 64) {
        const int m = 64 * c + lane;
        const int l = m < M ? lab[m] : 255;
        int rank = 0;
        for (int k = 0; k < K; ++k) {
            const unsigned long long mask = __ballot(l == k);
            if (l == k) rank = __popcll(mask & ((1ull << lane) - 1ull));
            if (lane == 0) ccnt[c * KP + k] = (unsigned short)__popcll(mask);
        }
        if (m < M) rnk[m] = (unsigned short)rank;
    }
    __syncthreads();
    if (wave == 0) {
        int run = 0;
        if (lane < K)
            for (int c = 0; c < chunks; ++c) {
                const int t = ccnt[c * KP + lane];
                ccnt[c * KP + lane] = (unsigned short)run;
                run += t;
            }
        int scan = run;
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(scan, o);
            if (lane >= o) scan += up;
        }
        if (lane < K) {
            cnt[lane] = run;
            off[lane] = scan - run;
        }
    }
    __syncthreads();
}
__device__ __forceinline__ int sorted_slot(int m, const unsigned char* lab, int KP, const unsigned short* rnk, const unsigned short* ccnt,
                                           const int* off) {
    const int l = lab[m];
    return off[l] + ccnt[(m >> 6) * KP + l] + rnk[m];
}
