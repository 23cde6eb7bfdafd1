// Scores of a whole oversampled set: M = R K_in sampled futures per agent, 1 <= M <= 4096, where the passes of frontend.hip / metrics.hip
// hold one sample per lane and stop at 64 (include/sttode_hip.h sttode_large_select / sttode_large_kde_nll / sttode_large_spread, DESIGN.md
// 4ac).  pred is round-major [R][n][K_in][Tf][2] -- the round buffer sttode_reduce_samples reads -- sample m = r K_in + k.
//   large_select_kernel    one workgroup per agent: ADE(a, m) / FDE(a, m) with bok_select_kernel's arithmetic for every sample, kept in LDS;
//                          the minimum and its lowest index over all samples and over each asked prefix; the values also go to the caller's
//                          workspace when segments are asked.
//   large_joint_kernel     one workgroup per segment: per sample the double sum of those values over the segment's agents, in agent order;
//                          the minimum over the samples and its lowest index.
//   large_kde_kernel       one workgroup per agent, frame after frame, float64: a thread keeps its <= 16 samples of the frame in registers
//                          through the four passes (mean, covariance, maximum, sum of exp).
//   large_spread_kernel    the M (M-1) / 2 pairs as tiles of 64 x 64 samples, a thread a 4 x 4 patch of one; a tile's samples go through LDS in
//                          blocks of frames; the tiles of an agent are dealt to up to 64 workgroups, whose partial sums go to the caller's
//                          workspace.  large_spread_finish adds them in workgroup order and forms the energy scores.
// Sum order, everywhere a sum runs over samples or pairs (wave_then_block_sum of set_body.hpp): a thread adds its own terms in ascending order (sample tid, tid + 256, ...; tiles
// g, g + G, ..., patch rows then columns), the 64 lanes of a wave are added by the xor tree 32, 16, ... 1, the four waves in wave order, the
// workgroups of an agent in workgroup order.  No atomics: two runs give the same bits, and an agent's or segment's values depend on nothing
// else in the batch (the number of workgroups per agent is a function of M alone).
#include <climits>
#include <cmath>

#include "api_util.hpp"
#include "set_body.hpp"
#include "../../include/sttode_hip.h"

namespace {

constexpr int LS_MAX_KS = 16;   // (MAX_M, MAX_TF: set_body.hpp, the sets sttode_reduce_samples takes)
constexpr int LS_SD = 4096;        // floats of the distance staging tile of large_select_kernel: min(256, 4096 / Tf) >= 20 samples per pass
constexpr int LK_PER = MAX_M / 256;   // samples per thread of large_kde_kernel
constexpr int SP_B = 64;           // samples per side of a pair tile
constexpr int SP_MAX_G = 64;       // workgroups per agent at most

struct LargeKs {
    int nk;
    int k[LS_MAX_KS];
};

// Minimum and lowest index of two value lists at once over the workgroup: wave xor tree, then the four waves in wave order (thread 0 holds
// the result).  red: 4 x 2 values and indices of LDS.
template <typename T>
__device__ __forceinline__ void block_argmin2(T& va, int& ia, T& vf, int& jf, T (*rv)[2], int (*ri)[2]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {   // (wave_take_lower's tree for both lists at once: the two chains of shuffles overlap)
        const T oa = __shfl_xor(va, o, 64), of = __shfl_xor(vf, o, 64);
        const int oia = __shfl_xor(ia, o, 64), oif = __shfl_xor(jf, o, 64);
        take_lower(va, ia, oa, oia);
        take_lower(vf, jf, of, oif);
    }
    __syncthreads();   // (the last use of rv / ri is over)
    if (lane == 0) {
        rv[w][0] = va;
        rv[w][1] = vf;
        ri[w][0] = ia;
        ri[w][1] = jf;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            take_lower(va, ia, rv[q][0], ri[q][0]);
            take_lower(vf, jf, rv[q][1], ri[q][1]);
        }
    }
}

// Per agent a = blockIdx.x.  Samples in passes of SC = min(256, LS_SD / Tf): the SC Tf displacement norms go into LDS by coalesced 8-byte
// reads (bok_dist), thread s < SC adds sample m0 + s's frames in frame order in fp32 and divides by Tf: the bits bok_select_kernel computes
// for that sample.  va / vf [M] stay in LDS.  A value wins a comparison only if it is smaller (<) than the best so far, which starts at
// +inf with index 0: NaN and +inf never win, and an agent without a finite sample gets +inf, index 0.
__global__ __launch_bounds__(256) void large_select_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int n, int K_in, int M,
                                                           int Tf, float scale, float thr, LargeKs ks, float* __restrict__ wsv,
                                                           float* __restrict__ ade, float* __restrict__ fde, int* __restrict__ ia,
                                                           int* __restrict__ ifd, unsigned char* __restrict__ miss, float* __restrict__ ade_at,
                                                           float* __restrict__ fde_at) {
    __shared__ float sd[LS_SD];
    __shared__ float2 sg[MAX_TF];
    __shared__ float va[MAX_M], vf[MAX_M];
    __shared__ float rv[4][2];
    __shared__ int ri[4][2];
    const int tid = threadIdx.x, a = blockIdx.x;
    const float2* p = reinterpret_cast<const float2*>(pred);
    const float2* g = reinterpret_cast<const float2*>(gt) + (size_t)a * Tf;
    for (int t = tid; t < Tf; t += 256) sg[t] = g[t];
    const int SC = min(256, LS_SD / Tf);
    for (int m0 = 0; m0 < M; m0 += SC) {
        const int sc = min(SC, M - m0);
        __syncthreads();   // (sg is written; the last pass's reads of sd are over)
        for (int e = tid; e < sc * Tf; e += 256) {
            const int s = e / Tf, t = e - s * Tf;
            const float2 v = p[round_major_row(a, m0 + s, n, K_in, Tf) + t], r = sg[t];
            sd[e] = bok_dist(v.x, v.y, r.x, r.y, scale);
        }
        __syncthreads();
        if (tid < sc) {
            float sum = 0.f;
            for (int t = 0; t < Tf; ++t) sum += sd[tid * Tf + t];
            va[m0 + tid] = sum / (float)Tf;
            vf[m0 + tid] = sd[tid * Tf + Tf - 1];
        }
    }
    __syncthreads();
    if (wsv) {
        float* wa = wsv + (size_t)a * M;
        float* wf = wsv + (size_t)n * M + (size_t)a * M;
        for (int m = tid; m < M; m += 256) {
            wa[m] = va[m];
            wf[m] = vf[m];
        }
    }
    // the prefixes in ascending order, the whole set last; a thread carries its best over from one prefix to the next
    float ba = INFINITY, bf = INFINITY;
    int ka = 0, kf = 0, done = 0;
    for (int q = 0; q <= ks.nk; ++q) {
        const int lim = q < ks.nk ? ks.k[q] : M;
        for (int m = done + ((tid - done) % 256 + 256) % 256; m < lim; m += 256) {   // the thread's samples m = tid (mod 256) in [done, lim)
            const float xa = va[m], xf = vf[m];
            if (xa < ba) {
                ba = xa;
                ka = m;
            }
            if (xf < bf) {
                bf = xf;
                kf = m;
            }
        }
        done = lim;
        float ma = ba, mf = bf;
        int ja = ka, jf = kf;
        block_argmin2(ma, ja, mf, jf, rv, ri);
        if (tid == 0) {
            if (q < ks.nk) {
                if (ade_at) ade_at[(size_t)a * ks.nk + q] = ma;
                if (fde_at) fde_at[(size_t)a * ks.nk + q] = mf;
            } else {
                ade[a] = ma;
                fde[a] = mf;
                if (ia) ia[a] = ja;
                if (ifd) ifd[a] = jf;
                if (miss) miss[a] = mf > thr ? 1 : 0;
            }
        }
    }
}

// Per segment s = blockIdx.x (bounds clamped to [0, n]): thread tid takes the samples m = tid, tid + 256, ...; per sample the double sum over
// the segment's agents of ADE(a, m) / FDE(a, m) (wsv: large_select_kernel's values), in agent order, divided by the agent count; the minimum
// over m of the double values (a sample with a NaN or infinite sum never wins) and its lowest index.  An empty segment gets NaN and -1, a
// segment without a finite sample +inf and 0.
__global__ __launch_bounds__(256) void large_joint_kernel(const float* __restrict__ wsv, int n, int M, const int* __restrict__ seg_ptr,
                                                          float* __restrict__ seg_jade, float* __restrict__ seg_jfde,
                                                          int* __restrict__ seg_jade_idx, int* __restrict__ seg_jfde_idx) {
    __shared__ double rv[4][2];
    __shared__ int ri[4][2];
    const int tid = threadIdx.x, s = blockIdx.x;
    int a0, a1;
    clamped_segment(seg_ptr, s, n, a0, a1);
    if (a1 == a0) {
        if (tid == 0) {
            seg_jade[s] = seg_jfde[s] = NAN;
            seg_jade_idx[s] = seg_jfde_idx[s] = -1;
        }
        return;
    }
    const float* wa = wsv;
    const float* wf = wsv + (size_t)n * M;
    const double c = (double)(a1 - a0);
    double ba = INFINITY, bf = INFINITY;
    int ka = 0, kf = 0;
    for (int m = tid; m < M; m += 256) {
        double sa = 0.0, sf = 0.0;
        for (int a = a0; a < a1; ++a) {
            sa += (double)wa[(size_t)a * M + m];
            sf += (double)wf[(size_t)a * M + m];
        }
        sa /= c;
        sf /= c;
        if (sa < ba) {
            ba = sa;
            ka = m;
        }
        if (sf < bf) {
            bf = sf;
            kf = m;
        }
    }
    block_argmin2(ba, ka, bf, kf, rv, ri);
    if (tid == 0) {
        seg_jade[s] = (float)ba;
        seg_jfde[s] = (float)bf;
        seg_jade_idx[s] = ka;
        seg_jfde_idx[s] = kf;
    }
}

// KDE NLL of agent a = blockIdx.x over its M samples (sttode_kde_nll's definition), frame after frame.  Thread tid holds the
// frame's samples m = tid + 256 j, j < LK_PER, raw, in registers; x = (double)(v * scale) with the product in fp32.  Four sums / one maximum
// over the samples per frame, each in the file's order: mean; unbiased covariance; the largest exponent; the sum of exp.  Every thread
// carries the same values, so the branch on a degenerate frame is uniform.
__global__ __launch_bounds__(256) void large_kde_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int n, int K_in, int M,
                                                        int Tf, float scale, double* __restrict__ nll) {
    __shared__ double red[4][3];
    const int tid = threadIdx.x, a = blockIdx.x;
    const float2* p = reinterpret_cast<const float2*>(pred);
    const float2* g = reinterpret_cast<const float2*>(gt) + (size_t)a * Tf;
    size_t base[LK_PER];
#pragma unroll
    for (int j = 0; j < LK_PER; ++j) base[j] = tid + 256 * j < M ? round_major_row(a, tid + 256 * j, n, K_in, Tf) : 0;
    const double f = pow((double)M, -1.0 / 6.0), f2 = f * f;
    const double logM = log((double)M);
    double acc = 0.0;
    bool bad = false;
    for (int t = 0; t < Tf; ++t) {
        float2 x[LK_PER];
#pragma unroll
        for (int j = 0; j < LK_PER; ++j) x[j] = tid + 256 * j < M ? p[base[j] + t] : make_float2(0.f, 0.f);
        double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < LK_PER; ++j)
            if (tid + 256 * j < M) {
                s[0] += (double)(x[j].x * scale);
                s[1] += (double)(x[j].y * scale);
            }
        wave_then_block_sum<3>(s, red);
        const double mx = s[0] / M, my = s[1] / M;
        double c[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < LK_PER; ++j)
            if (tid + 256 * j < M) {
                const double dx = (double)(x[j].x * scale) - mx, dy = (double)(x[j].y * scale) - my;
                c[0] += dx * dx;
                c[1] += dx * dy;
                c[2] += dy * dy;
            }
        wave_then_block_sum<3>(c, red);
        const double c00 = c[0] / (M - 1), c01 = c[1] / (M - 1), c11 = c[2] / (M - 1);
        double det, inv;
        if (!kde_cov(c00, c01, c11, f2, det, inv)) {
            bad = true;
            continue;
        }
        const float2 r = g[t];
        const double gx = (double)(r.x * scale), gy = (double)(r.y * scale);
        double e[LK_PER];
        double mxe = -INFINITY;
#pragma unroll
        for (int j = 0; j < LK_PER; ++j)
            if (tid + 256 * j < M) {
                const double dx = gx - (double)(x[j].x * scale), dy = gy - (double)(x[j].y * scale);
                e[j] = -0.5 * kde_quad(c00, c01, c11, inv, dx, dy);
                mxe = fmax(mxe, e[j]);
            }
        mxe = wave_max(mxe);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6][0] = mxe;
        __syncthreads();
        mxe = fmax(fmax(red[0][0], red[1][0]), fmax(red[2][0], red[3][0]));
        double se[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < LK_PER; ++j)
            if (tid + 256 * j < M) se[0] += exp(e[j] - mxe);
        wave_then_block_sum<3>(se, red);
        acc += kde_clip(log(se[0]) + mxe - logM - kde_log_norm(f2, det));
    }
    if (tid == 0) nll[a] = bad ? (double)NAN : -acc / Tf;
}

// Tiles of an agent's pair space: NB = ceil(M / 64) blocks of samples, the tiles (ib, jb) with ib <= jb in row order, NB (NB + 1) / 2 of
// them; G = min(tiles, SP_MAX_G) workgroups per agent.  Host and device agree through these two functions.
__host__ __device__ inline int spread_tiles(int M) {
    const int nb = (M + SP_B - 1) / SP_B;
    return nb * (nb + 1) / 2;
}
__host__ __device__ inline int spread_groups(int M) { return spread_tiles(M) < SP_MAX_G ? spread_tiles(M) : SP_MAX_G; }

// Workgroup blockIdx.x = a G + g: the tiles g, g + G, ... of agent a.  In a tile thread tid holds the 4 x 4 pairs (i, j) = (64 ib + ti + 16 u,
// 64 jb + tj + 16 v), ti = tid / 16, tj = tid % 16: per pair the running sum of squared distances and of distances, frames in frame order;
// the two blocks of samples go through LDS SET_FT frames at a time (raw float2; x = (double)(v * scale), everything after that float64, as
// sample_spread_kernel).  The last frame's distance goes straight into the thread's final-distance sum.  After the last frame the valid
// pairs (i < j < M) are finished in (u, v) order into the thread's four sums; after the last tile those are added over the workgroup and
// stored as part[(a G + g) 4 + q], q = trajectory distance, final distance, mean frame distance, DLow kernel value.
__global__ __launch_bounds__(256) void large_spread_kernel(const float* __restrict__ pred, int n, int K_in, int M, int Tf, float scale,
                                                           double div_scale, double* __restrict__ part) {
    __shared__ float2 xi[SP_B * SET_STRIDE], xj[SP_B * SET_STRIDE];
    __shared__ double red[4][4];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int G = spread_groups(M), T = spread_tiles(M), NB = (M + SP_B - 1) / SP_B;
    const int a = blockIdx.x / G, g = blockIdx.x - a * G;
    const float2* p = reinterpret_cast<const float2*>(pred);
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    for (int tile = g; tile < T; tile += G) {
        int ib, jb;   // the tiles in row order with ib <= jb: the pairs (ib, jb + 1) of NB + 1 items
        pdist_pair(tile, NB + 1, ib, jb);
        --jb;
        double s2[4][4], s1[4][4];
        bool ok[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                s2[u][v] = s1[u][v] = 0.0;
                const int i = SP_B * ib + ti + 16 * u, j = SP_B * jb + tj + 16 * v;
                ok[u][v] = i < j && j < M;
            }
        for (int t0 = 0; t0 < Tf; t0 += SET_FT) {
            const int ft = min(SET_FT, Tf - t0);
            __syncthreads();   // (the last block's reads are over)
            for (int e = tid; e < SP_B * ft; e += 256) {
                const int s = e / ft, tl = e - s * ft;
                const int mi = SP_B * ib + s, mj = SP_B * jb + s;
                xi[s * SET_STRIDE + tl] = mi < M ? p[round_major_row(a, mi, n, K_in, Tf) + t0 + tl] : make_float2(0.f, 0.f);
                xj[s * SET_STRIDE + tl] = mj < M ? p[round_major_row(a, mj, n, K_in, Tf) + t0 + tl] : make_float2(0.f, 0.f);
            }
            __syncthreads();
            for (int tl = 0; tl < ft; ++tl) {
                double ax[4], ay[4], bx[4], by[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float2 vi = xi[(ti + 16 * u) * SET_STRIDE + tl], vj = xj[(tj + 16 * u) * SET_STRIDE + tl];
                    ax[u] = (double)(vi.x * scale);
                    ay[u] = (double)(vi.y * scale);
                    bx[u] = (double)(vj.x * scale);
                    by[u] = (double)(vj.y * scale);
                }
                const bool last = t0 + tl == Tf - 1;
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const double dx = ax[u] - bx[v], dy = ay[u] - by[v];
                        const double d2 = dx * dx + dy * dy;
                        const double d = sqrt(d2);
                        s2[u][v] += d2;
                        s1[u][v] += d;
                        if (last && ok[u][v]) tot[1] += d;
                    }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (ok[u][v]) {
                    tot[0] += sqrt(s2[u][v]);
                    tot[2] += s1[u][v] / Tf;
                    tot[3] += exp(-s2[u][v] / div_scale);
                }
    }
    wave_then_block_sum<4>(tot, red);
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) part[(size_t)blockIdx.x * 4 + q] = tot[q];
    }
}

// Per agent a = blockIdx.x: the G partial sums in workgroup order, divided by the pair count; with gt the float64 mean-over-frames and
// last-frame distance of every sample to the ground truth (thread tid: m = tid, tid + 256, ..., frames in frame order), added in the
// file's order, for the energy scores es = (1/M) sum_m D(x_m, y) - ((M-1) / (2M)) (mean pair distance).
__global__ __launch_bounds__(256) void large_spread_finish(const float* __restrict__ pred, const float* __restrict__ gt, int n, int K_in, int M,
                                                           int Tf, float scale, const double* __restrict__ part, double* __restrict__ apd,
                                                           double* __restrict__ fpd, double* __restrict__ pade, double* __restrict__ dlow,
                                                           double* __restrict__ es_ade, double* __restrict__ es_fde) {
    __shared__ double red[4][2];
    const int tid = threadIdx.x, a = blockIdx.x, G = spread_groups(M);
    double gs[2] = {0.0, 0.0};
    if (gt) {   // (uniform)
        const float2* p = reinterpret_cast<const float2*>(pred);
        const float2* g = reinterpret_cast<const float2*>(gt) + (size_t)a * Tf;
        for (int m = tid; m < M; m += 256) {
            const float2* x = p + round_major_row(a, m, n, K_in, Tf);
            double sum = 0.0, d = 0.0;
            for (int t = 0; t < Tf; ++t) {
                const float2 v = x[t], y = g[t];
                const double dx = (double)(v.x * scale) - (double)(y.x * scale), dy = (double)(v.y * scale) - (double)(y.y * scale);
                d = sqrt(dx * dx + dy * dy);
                sum += d;
            }
            gs[0] += sum / Tf;
            gs[1] += d;
        }
        wave_then_block_sum<2>(gs, red);
    }
    if (tid != 0) return;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] += part[((size_t)a * G + g) * 4 + q];
    const double np = 0.5 * (double)M * (double)(M - 1), c = (double)(M - 1) / (2.0 * M);
    apd[a] = v[0] / np;
    fpd[a] = v[1] / np;
    pade[a] = v[2] / np;
    dlow[a] = v[3] / np;
    if (es_ade) es_ade[a] = gs[0] / M - c * (v[2] / np);
    if (es_fde) es_fde[a] = gs[1] / M - c * (v[1] / np);
}

// The checks the three entries share: nullptr, or why not.  M_min: the smallest M the entry takes.
const char* large_shape_check(int n, int R, int K_in, int Tf, int M_min) {
    if (n < 1) return "n must be positive";
    if (R < 1 || K_in < 1 || R > MAX_M || K_in > MAX_M || R * K_in > MAX_M) return "needs 1 <= M = R K_in <= 4096 (R, K_in >= 1)";
    if (R * K_in < M_min) return M_min == 3 ? "needs M = R K_in >= 3 (two points are collinear: no covariance)" : "needs M = R K_in >= 2 (a pair)";
    if (Tf < 1 || Tf > MAX_TF) return "Tf must be in [1, 200]";
    return nullptr;
}

}  // namespace

extern "C" long long int sttode_large_select_ws(int n, int M) {
    if (n < 1 || M < 1 || M > MAX_M) {
        stt_set_error("sttode_large_select_ws: needs n >= 1 and 1 <= M <= 4096");
        return -1;
    }
    return 2ll * n * M * (long long)sizeof(float);
}

extern "C" int sttode_large_select(const float* pred, const float* gt, int n, int R, int K_in, int Tf, float scale, float miss_threshold,
                                   const int* ks, int nk, const int* seg_ptr, int S, void* ws, long ws_bytes, float* ade, float* fde,
                                   int* best_ade_idx, int* best_fde_idx, unsigned char* miss, float* ade_at, float* fde_at, float* seg_jade,
                                   float* seg_jfde, int* seg_jade_idx, int* seg_jfde_idx, void* stream) {
    const char* who = "sttode_large_select";
    if (!(pred && gt && ade && fde)) return stt_refuse(who, "null pointer (pred, gt, ade and fde are required)");
    if (const char* why = large_shape_check(n, R, K_in, Tf, 1)) return stt_refuse(who, why);
    const int M = R * K_in;
    LargeKs kk = {};
    if (nk < 0 || nk > LS_MAX_KS) return stt_refuse(who, "nk must be in [0, 16]");
    if (nk > 0 && !(ks && ade_at && fde_at)) return stt_refuse(who, "null pointer (nk > 0 needs ks, ade_at and fde_at)");
    if (nk == 0 && (ade_at || fde_at)) return stt_refuse(who, "ade_at and fde_at need ks (pass them as NULL with nk = 0)");
    for (int i = 0; i < nk; ++i) {
        if (ks[i] < 1 || ks[i] > M || (i > 0 && ks[i] <= ks[i - 1])) return stt_refuse(who, "ks must be strictly ascending in [1, M]");
        kk.k[i] = ks[i];
    }
    kk.nk = nk;
    const bool segs = seg_ptr || seg_jade || seg_jfde || seg_jade_idx || seg_jfde_idx;
    if (segs) {
        if (!(seg_ptr && seg_jade && seg_jfde && seg_jade_idx && seg_jfde_idx))
            return stt_refuse(who, "null pointer (the joint outputs need seg_ptr, seg_jade, seg_jfde, seg_jade_idx and seg_jfde_idx together)");
        if (S < 1) return stt_refuse(who, "S must be positive with seg_ptr");
        if (!ws || ws_bytes < sttode_large_select_ws(n, M))
            return stt_refuse(who, "the joint outputs need a workspace of sttode_large_select_ws(n, M) bytes");
    }
    hipStream_t st = (hipStream_t)stream;
    float* wsv = segs ? (float*)ws : nullptr;
    hipLaunchKernelGGL(large_select_kernel, dim3(n), dim3(256), 0, st, pred, gt, n, K_in, M, Tf, scale, miss_threshold, kk, wsv, ade, fde,
                       best_ade_idx, best_fde_idx, miss, ade_at, fde_at);
    if (segs)
        hipLaunchKernelGGL(large_joint_kernel, dim3(S), dim3(256), 0, st, (const float*)wsv, n, M, seg_ptr, seg_jade, seg_jfde, seg_jade_idx,
                           seg_jfde_idx);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_large_kde_nll(const float* pred, const float* gt, int n, int R, int K_in, int Tf, float scale, double* nll,
                                    void* stream) {
    const char* who = "sttode_large_kde_nll";
    if (!(pred && gt && nll)) return stt_refuse(who, "null pointer (pred, gt and nll are required)");
    if (const char* why = large_shape_check(n, R, K_in, Tf, 3)) return stt_refuse(who, why);
    hipLaunchKernelGGL(large_kde_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, pred, gt, n, K_in, R * K_in, Tf, scale, nll);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" long long int sttode_large_spread_ws(int n, int M) {
    if (n < 1 || M < 2 || M > MAX_M || (long long)n * spread_groups(M) > INT_MAX) {
        stt_set_error("sttode_large_spread_ws: needs n >= 1, 2 <= M <= 4096 and n * min(tiles, 64) workgroups below 2^31");
        return -1;
    }
    return 4ll * n * spread_groups(M) * (long long)sizeof(double);
}

extern "C" int sttode_large_spread(const float* pred, const float* gt, int n, int R, int K_in, int Tf, float scale, double div_scale, void* ws,
                                   long ws_bytes, double* apd, double* fpd, double* pade, double* dlow, double* es_ade, double* es_fde,
                                   void* stream) {
    const char* who = "sttode_large_spread";
    if (!(pred && apd && fpd && pade && dlow)) return stt_refuse(who, "null pointer (pred, apd, fpd, pade and dlow are required)");
    if (!gt && (es_ade || es_fde)) return stt_refuse(who, "es_ade and es_fde need gt (pass them as NULL without it)");
    if (const char* why = large_shape_check(n, R, K_in, Tf, 2)) return stt_refuse(who, why);
    if (!(div_scale > 0.0) || std::isinf(div_scale)) return stt_refuse(who, "div_scale must be positive and finite");
    const int M = R * K_in, G = spread_groups(M);
    if ((long long)n * G > INT_MAX) return stt_refuse(who, "n is too large (n * min(tiles, 64) workgroups must stay below 2^31)");
    if (!ws || ws_bytes < sttode_large_spread_ws(n, M)) return stt_refuse(who, "needs a workspace of sttode_large_spread_ws(n, M) bytes");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(large_spread_kernel, dim3(n * G), dim3(256), 0, st, pred, n, K_in, M, Tf, scale, div_scale, (double*)ws);
    hipLaunchKernelGGL(large_spread_finish, dim3(n), dim3(256), 0, st, pred, gt, n, K_in, M, Tf, scale, (const double*)ws, apd, fpd, pade, dlow,
                       es_ade, es_fde);
    STT_HIP(hipGetLastError());
    return 0;
}
