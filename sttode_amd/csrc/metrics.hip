// Scene-level metrics of K sampled futures: joint (one sample index per segment) min ADE / FDE, the collision rate of the predictions and of
// the ground truth, and the KDE negative log-likelihood of the ground truth (Trajectron++'s compute_kde_nll).  The reference prints none of
// these; the definitions are those of include/sttode_hip.h (sttode_joint_select, sttode_kde_nll) and DESIGN.md §4l.
//   joint_select_kernel     one workgroup per segment: per-(agent, sample) ADE / FDE with bok_select_kernel's arithmetic, a double sum per
//                           sample over the segment's agents, the lowest-index minimum.
//   joint_collision_kernel  one workgroup per segment: per sample (and the ground truth) the agents that come closer than r to another agent
//                           of the segment at some frame; positions staged in LDS in tiles of 64 agents x 8 frames.
//   kde_nll_kernel          one wave per agent, frames on lanes, everything in float64; samples staged in LDS in tiles of frames.
//   sample_spread_kernel    one workgroup per agent: the K (K-1) / 2 sample pairs dealt to the threads, float64 (sttode_sample_spread, 4s).
// No atomics: every sum has a fixed order, so runs give the same bits.
#include <cmath>

#include "api_util.hpp"
#include "set_body.hpp"
#include "../../include/sttode_hip.h"

namespace {

constexpr int COL_FT = 8;   // frames per LDS tile of the collision pass (a wave's two tiles: 2 x 64 agents x 8 frames x float2 = 8 KiB)

// Per segment s (agents seg_ptr[s] .. seg_ptr[s+1]-1, bounds clamped to [0, n]): wave w takes the agents a0 + w, a0 + w + 4, ...; lane k
// computes ADE(a, k) / FDE(a, k) exactly as bok_select_kernel does (the K Tf distances through LDS by coalesced 8-byte reads when K Tf <= 1024,
// frames summed in order in fp32, divided by Tf) and adds them to a double partial.  The four waves' partials are added in wave order, the
// sums divided by the agent count; the minimum over k (NaN samples skipped) and its lowest index (a ballot: np.argmin's rule on exact ties).
// The double sums of fp32 values are exact whenever the values span less than 2^19 in magnitude and the segment has at most 1024 agents, so
// the order of the partials then does not show in the bits.  An empty segment (or one whose samples are all NaN) gets NaN and index 0.
__global__ __launch_bounds__(256) void joint_select_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int n, int K, int Tf,
                                                           float scale, const int* __restrict__ seg_ptr, float* __restrict__ seg_jade,
                                                           float* __restrict__ seg_jfde, int* __restrict__ seg_jade_idx,
                                                           int* __restrict__ seg_jfde_idx) {
    __shared__ float sd[4][1024];
    __shared__ double part[2][4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int s = blockIdx.x;
    int a0, a1;
    clamped_segment(seg_ptr, s, n, a0, a1);
    const int tot = K * Tf;
    double pa = 0.0, pf = 0.0;
    for (int a = a0 + w; a < a1; a += 4) {
        const float2* g = reinterpret_cast<const float2*>(gt + (size_t)a * Tf * 2);
        const float2* p = reinterpret_cast<const float2*>(pred + (size_t)a * K * Tf * 2);
        float va = 0.f, vf = 0.f;
        if (tot <= 1024) {
            for (int i = lane; i < tot; i += 64) {
                const float2 v = p[i], r = g[i % Tf];
                sd[w][i] = bok_dist(v.x, v.y, r.x, r.y, scale);
            }
            __builtin_amdgcn_wave_barrier();
            if (lane < K) {
                float sum = 0.f;
                for (int t = 0; t < Tf; ++t) sum += sd[w][lane * Tf + t];
                va = sum / (float)Tf;
                vf = sd[w][lane * Tf + Tf - 1];
            }
            __builtin_amdgcn_wave_barrier();   // (the next agent's distances overwrite sd[w])
        } else if (lane < K) {
            float sum = 0.f, dl = 0.f;
            for (int t = 0; t < Tf; ++t) {
                const float2 v = p[lane * Tf + t], r = g[t];
                dl = bok_dist(v.x, v.y, r.x, r.y, scale);
                sum += dl;
            }
            va = sum / (float)Tf;
            vf = dl;
        }
        pa += (double)va;
        pf += (double)vf;
    }
    part[0][w][lane] = pa;
    part[1][w][lane] = pf;
    __syncthreads();
    if (w != 0) return;
    const double c = (double)(a1 - a0);
    double va = INFINITY, vf = INFINITY;
    if (lane < K) {
        va = (((part[0][0][lane] + part[0][1][lane]) + part[0][2][lane]) + part[0][3][lane]) / c;
        vf = (((part[1][0][lane] + part[1][1][lane]) + part[1][2][lane]) + part[1][3][lane]) / c;
    }
    const double ma = wave_min(va), mf = wave_min(vf);
    const unsigned long long ba = __ballot(lane < K && va == ma), bf = __ballot(lane < K && vf == mf);
    if (lane == 0) {
        seg_jade[s] = ba ? (float)ma : NAN;
        seg_jfde[s] = bf ? (float)mf : NAN;
        seg_jade_idx[s] = ba ? __builtin_ctzll(ba) : 0;
        seg_jfde_idx[s] = bf ? __builtin_ctzll(bf) : 0;
    }
}

// Per segment s: for every sample k < K and for the ground truth (k = K), the number of agents a of the segment for which some other agent b
// of the segment has dx^2 + dy^2 < r2 at some frame (dx, dy: fp32 differences of the scaled coordinates; fma(dx, dx, dy * dy) as bok_dist).
// Work units (k, block of 64 agents) are dealt to the four waves; lane = agent of the block.  Per tile of COL_FT frames a unit stages its own
// block's positions (mine) and then each block of 64 agents of the segment (tile) in the wave's own LDS, scaled, and ORs its per-agent flag
// over the frames; it stops once every agent of its block has collided.  seg_col[s] = sum over k < K of the colliding agents, seg_gt_col[s]
// = those of the ground truth.
__global__ __launch_bounds__(256) void joint_collision_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int n, int K, int Tf,
                                                              float scale, const int* __restrict__ seg_ptr, float r2, int* __restrict__ seg_col,
                                                              int* __restrict__ seg_gt_col) {
    __shared__ float2 tile[4][COL_FT][64];
    __shared__ float2 mine[4][COL_FT][64];
    __shared__ int cnt[4][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int s = blockIdx.x;
    int a0, a1;
    clamped_segment(seg_ptr, s, n, a0, a1);
    const int na = a1 - a0, nblk = (na + 63) / 64;
    int col = 0, gcol = 0;
    for (int u = w; u < (K + 1) * nblk; u += 4) {
        const int k = u / nblk, blk = u - k * nblk;
        const float* base = k < K ? pred + (size_t)k * Tf * 2 : gt;                  // agent a0 + i of sample k: base + (a0 + i) * rs
        const size_t rs = k < K ? (size_t)K * Tf * 2 : (size_t)Tf * 2;
        const int ia = blk * 64 + lane;
        const bool own = ia < na;
        const int nm = min(64, na - blk * 64);
        bool hit = false;
        for (int t0 = 0; t0 < Tf && __ballot(own && !hit) != 0; t0 += COL_FT) {
            const int ft = min(COL_FT, Tf - t0);
            for (int i = lane; i < nm * ft; i += 64) {
                const int b = i / ft, tl = i - b * ft;
                const float2 v = *reinterpret_cast<const float2*>(base + (size_t)(a0 + blk * 64 + b) * rs + (size_t)(t0 + tl) * 2);
                mine[w][tl][b] = make_float2(v.x * scale, v.y * scale);
            }
            for (int bb = 0; bb < nblk; ++bb) {
                const int nb = min(64, na - bb * 64);
                for (int i = lane; i < nb * ft; i += 64) {
                    const int b = i / ft, tl = i - b * ft;
                    const float2 v = *reinterpret_cast<const float2*>(base + (size_t)(a0 + bb * 64 + b) * rs + (size_t)(t0 + tl) * 2);
                    tile[w][tl][b] = make_float2(v.x * scale, v.y * scale);
                }
                __builtin_amdgcn_wave_barrier();
                if (own) {
                    for (int tl = 0; tl < ft && !hit; ++tl) {
                        const float2 q = mine[w][tl][lane];
                        for (int b = 0; b < nb; ++b) {
                            const float2 o = tile[w][tl][b];
                            const float dx = q.x - o.x, dy = q.y - o.y;
                            hit |= (bb * 64 + b != ia) && __fmaf_rn(dx, dx, dy * dy) < r2;
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();   // (the next tile overwrites tile[w] and mine[w])
                if (__ballot(own && !hit) == 0) break;
            }
        }
        const int c = __popcll(__ballot(own && hit));
        if (k < K) col += c;
        else gcol += c;
    }
    if (lane == 0) {
        cnt[w][0] = col;
        cnt[w][1] = gcol;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        seg_col[s] = cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0];
        seg_gt_col[s] = cnt[0][1] + cnt[1][1] + cnt[2][1] + cnt[3][1];
    }
}

// KDE NLL of agent a (Trajectron++ compute_kde_nll over scipy.stats.gaussian_kde), one wave per agent.  Lane t of a frame tile handles frame
// t0 + t: x_k = (double)(pred * scale) (the fp32 product), mean and unbiased covariance C over the K samples in sample order, Scott's factor
// f = K^(-1/6), Sigma = f^2 C with the closed-form 2 x 2 inverse and determinant, logsumexp over k in two passes (max, then the sum of exp),
// logpdf = lse - log K - log det(2 pi Sigma) / 2, clipped below at -20.  The frames' values are added by a fixed xor tree per tile and the
// tiles in order; nll = -sum / Tf.  A frame with C00 <= 0 or det C <= 0 (not positive definite, where gaussian_kde raises) makes nll NaN.
// The wave's samples go through its own LDS tile of 1024 float2 (K samples x min(64, 1024 / K) frames).
__global__ __launch_bounds__(256) void kde_nll_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int n, int K, int Tf,
                                                      float scale, double* __restrict__ nll) {
    __shared__ float2 sx[4][1024];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int a = blockIdx.x * 4 + w;
    if (a >= n) return;
    const float2* p = reinterpret_cast<const float2*>(pred + (size_t)a * K * Tf * 2);
    const float2* g = reinterpret_cast<const float2*>(gt + (size_t)a * Tf * 2);
    const int ftm = min(64, 1024 / K);
    const double f = pow((double)K, -1.0 / 6.0), f2 = f * f;
    const double logK = log((double)K);
    double acc = 0.0;
    bool bad = false;
    for (int t0 = 0; t0 < Tf; t0 += ftm) {
        const int ft = min(ftm, Tf - t0);
        for (int i = lane; i < K * ft; i += 64) {
            const int k = i / ft, tl = i - k * ft;
            sx[w][i] = p[k * Tf + t0 + tl];
        }
        __builtin_amdgcn_wave_barrier();
        double lp = 0.0;
        if (lane < ft) {
            double mx = 0.0, my = 0.0;
            for (int k = 0; k < K; ++k) {
                const float2 v = sx[w][k * ft + lane];
                mx += (double)(v.x * scale);
                my += (double)(v.y * scale);
            }
            mx /= K;
            my /= K;
            double c00 = 0.0, c01 = 0.0, c11 = 0.0;
            for (int k = 0; k < K; ++k) {
                const float2 v = sx[w][k * ft + lane];
                const double dx = (double)(v.x * scale) - mx, dy = (double)(v.y * scale) - my;
                c00 += dx * dx;
                c01 += dx * dy;
                c11 += dy * dy;
            }
            c00 /= (K - 1);
            c01 /= (K - 1);
            c11 /= (K - 1);
            double det, inv;
            if (!kde_cov(c00, c01, c11, f2, det, inv)) {
                bad = true;
            } else {
                const float2 r = g[t0 + lane];
                const double gx = (double)(r.x * scale), gy = (double)(r.y * scale);
                double m = -INFINITY;
                for (int k = 0; k < K; ++k) {
                    const float2 v = sx[w][k * ft + lane];
                    const double dx = gx - (double)(v.x * scale), dy = gy - (double)(v.y * scale);
                    m = fmax(m, -0.5 * kde_quad(c00, c01, c11, inv, dx, dy));
                }
                double sum = 0.0;
                for (int k = 0; k < K; ++k) {
                    const float2 v = sx[w][k * ft + lane];
                    const double dx = gx - (double)(v.x * scale), dy = gy - (double)(v.y * scale);
                    sum += exp(-0.5 * kde_quad(c00, c01, c11, inv, dx, dy) - m);
                }
                lp = kde_clip(log(sum) + m - logK - kde_log_norm(f2, det));
            }
        }
        acc += wave_sum(lp);
        __builtin_amdgcn_wave_barrier();   // (the next tile overwrites sx[w])
    }
    const bool any_bad = __ballot(bad) != 0;
    if (lane == 0) nll[a] = any_bad ? (double)NAN : -acc / Tf;
}

// Spread of agent a's K samples among themselves (include/sttode_hip.h sttode_sample_spread), one workgroup per agent.
// Coordinates are (double)(x * scale) with the product in fp32, everything after that float64.  The samples go through LDS in tiles of SET_FT
// frames (raw float2, rows of SET_STRIDE).  Pair p (F.pdist order: (0,1), (0,2), ... (K-2,K-1)) belongs to thread p mod 256; a thread keeps, per
// pair, the running sum of squared distances, the running sum of distances and the last frame's distance, frames in frame order.  After the
// last tile it finishes its pairs in pair order (sqrt, exp) into four partial sums; those go through LDS, wave 0 adds the four of lane l,
// l + 64, l + 128, l + 192 in that order and the 64 lanes by a fixed xor tree.  No atomics.
// R = pairs per thread, KM = the largest K.  <8, 64> takes any K (2016 pairs <= 8 * 256); <1, SET_K1> is the same code for K <= 23, where the
// registers of seven more pairs and the LDS of 41 more samples would halve the workgroups a CU holds: the kernel waits on latency.
// With gt: wave 3 (the one with the fewest pairs), lane = sample, sums the float64 distances to the ground truth for the energy scores and, in
// fp32 with bok_dist in frame order, bok_select_kernel's ADE(a, k) / FDE(a, k); an inclusive prefix minimum over the lanes (fminf: NaN
// skipped) gives the *_at_k rows.  A prefix of k < 64 samples that are all NaN gives +inf (k = 64: NaN), as the selection of those k samples.
template <int R, int KM>
__global__ __launch_bounds__(256) void sample_spread_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int K, int Tf,
                                                            float scale, double div_scale, double* __restrict__ apd, double* __restrict__ fpd,
                                                            double* __restrict__ pade, double* __restrict__ dlow, double* __restrict__ es_ade,
                                                            double* __restrict__ es_fde, float* __restrict__ ade_at_k,
                                                            float* __restrict__ fde_at_k) {
    __shared__ float2 sx[KM * SET_STRIDE];
    __shared__ float2 sg[SET_FT];
    __shared__ double red[4][256];
    __shared__ double gsum[2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int a = blockIdx.x;
    const int P = K * (K - 1) / 2;
    const float2* p = reinterpret_cast<const float2*>(pred + (size_t)a * K * Tf * 2);
    const float2* g = gt ? reinterpret_cast<const float2*>(gt + (size_t)a * Tf * 2) : nullptr;
    int ij[R];                                   // (i, j) of the thread's r-th pair as i | j << 8
    double s2[R], s1[R], dl[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int q = tid + 256 * r, i = 0;
        if (q < P) i = pdist_row(q, K);
        ij[r] = i | (i + 1 + q) << 8;
        s2[r] = s1[r] = dl[r] = 0.0;
    }
    const bool gw = g != nullptr && w == 3;
    double ga = 0.0, gl = 0.0;                            // wave 3, lane k: sum over frames of |x_k - y| and the last frame's, float64
    float fa = 0.f, fl = 0.f;                             // the same with bok_dist in fp32
    for (int t0 = 0; t0 < Tf; t0 += SET_FT) {
        const int ft = min(SET_FT, Tf - t0);
        stage_tile<int>(sx, sg, p, g, K, Tf, t0, ft, tid);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (tid + 256 * r < P) pair_tile_accumulate(sx, ij[r], ft, scale, s2[r], s1[r], dl[r]);
        if (gw && lane < K) gt_tile_accumulate(sx, sg, lane, ft, scale, ga, gl, fa, fl);
        __syncthreads();   // (the next tile overwrites sx and sg)
    }
    double t_apd = 0.0, t_fpd = 0.0, t_pade = 0.0, t_dlow = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (tid + 256 * r < P) {
            t_apd += sqrt(s2[r]);
            t_fpd += dl[r];
            t_pade += s1[r] / Tf;
            t_dlow += exp(-s2[r] / div_scale);
        }
    }
    red[0][tid] = t_apd;
    red[1][tid] = t_fpd;
    red[2][tid] = t_pade;
    red[3][tid] = t_dlow;
    if (gw) {
        const double da = wave_sum(lane < K ? ga / Tf : 0.0), df = wave_sum(lane < K ? gl : 0.0);
        if (lane == 0) {
            gsum[0] = da;
            gsum[1] = df;
        }
        if (ade_at_k || fde_at_k) {
            const float va = prefix_fmin64(lane < K ? fa / (float)Tf : INFINITY, lane), vf = prefix_fmin64(lane < K ? fl : INFINITY, lane);
            if (lane < K) {
                if (ade_at_k) ade_at_k[(size_t)a * K + lane] = va;
                if (fde_at_k) fde_at_k[(size_t)a * K + lane] = vf;
            }
        }
    }
    __syncthreads();
    if (w != 0) return;
    double v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = quad_then_wave_sum(red[q], lane);
    if (lane == 0) {
        const double np = (double)P, c = (double)(K - 1) / (2.0 * K);
        apd[a] = v[0] / np;
        fpd[a] = v[1] / np;
        pade[a] = v[2] / np;
        dlow[a] = v[3] / np;
        if (es_ade) es_ade[a] = gsum[0] / K - c * (v[2] / np);
        if (es_fde) es_fde[a] = gsum[1] / K - c * (v[1] / np);
    }
}

}  // namespace

// Argument checks of the joint pass, shared with sttode_async_joint_select (pipeline.hip): 0, or 1 with the error set naming `who`.
int stt_joint_check(const char* who, const float* pred, const float* gt, int n, int K, int Tf, const int* seg_ptr, int S, float radius,
                    const float* seg_jade, const float* seg_jfde, const int* seg_jade_idx, const int* seg_jfde_idx, const int* seg_col,
                    const int* seg_gt_col) {
    const char* why = nullptr;
    if (!(pred && gt && seg_ptr && seg_jade && seg_jfde && seg_jade_idx && seg_jfde_idx))
        why = "null pointer (pred, gt, seg_ptr and the four joint outputs are required)";
    else if (radius > 0.f && !(seg_col && seg_gt_col))
        why = "null pointer (radius > 0 needs seg_col and seg_gt_col)";
    else if (!(n > 0 && K > 0 && Tf > 0 && S > 0))
        why = "n, K, Tf and S must be positive";
    else if (K > 64)
        why = "K > 64 is not supported (one lane per sample)";
    return why ? stt_refuse(who, why) : 0;
}

int stt_kde_check(const char* who, const float* pred, const float* gt, int n, int K, int Tf, const double* nll) {
    const char* why = nullptr;
    if (!(pred && gt && nll))
        why = "null pointer (pred, gt and nll are required)";
    else if (!(n > 0 && Tf > 0))
        why = "n and Tf must be positive";
    else if (K < 2 || K > 64)
        why = "needs 2 <= K <= 64 (K < 2: no covariance; K > 64: one LDS tile per frame block)";
    return why ? stt_refuse(who, why) : 0;
}

int stt_spread_check(const char* who, const float* pred, const float* gt, int n, int K, int Tf, double div_scale, const double* apd,
                     const double* fpd, const double* pade, const double* dlow, const double* es_ade, const double* es_fde,
                     const float* ade_at_k, const float* fde_at_k) {
    const char* why = nullptr;
    if (!(pred && apd && fpd && pade && dlow))
        why = "null pointer (pred, apd, fpd, pade and dlow are required)";
    else if (!gt && (es_ade || es_fde || ade_at_k || fde_at_k))
        why = "es_ade, es_fde, ade_at_k and fde_at_k need gt (pass them as NULL without it)";
    else if (!(n > 0 && Tf > 0))
        why = "n and Tf must be positive";
    else if (K < 2 || K > 64)
        why = "needs 2 <= K <= 64 (K < 2: no pair; K > 64: one lane per sample)";
    else if (!(div_scale > 0.0) || std::isinf(div_scale))
        why = "div_scale must be positive and finite";
    return why ? stt_refuse(who, why) : 0;
}

extern "C" int sttode_joint_select(const float* pred, const float* gt, int n, int K, int Tf, float scale, const int* seg_ptr, int S, float radius,
                                   float* seg_jade, float* seg_jfde, int* seg_jade_idx, int* seg_jfde_idx, int* seg_col, int* seg_gt_col,
                                   void* stream) {
    if (stt_joint_check("sttode_joint_select", pred, gt, n, K, Tf, seg_ptr, S, radius, seg_jade, seg_jfde, seg_jade_idx, seg_jfde_idx, seg_col,
                        seg_gt_col))
        return 1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(joint_select_kernel, dim3(S), dim3(256), 0, st, pred, gt, n, K, Tf, scale, seg_ptr, seg_jade, seg_jfde, seg_jade_idx,
                       seg_jfde_idx);
    if (radius > 0.f)
        hipLaunchKernelGGL(joint_collision_kernel, dim3(S), dim3(256), 0, st, pred, gt, n, K, Tf, scale, seg_ptr, radius * radius, seg_col,
                           seg_gt_col);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_kde_nll(const float* pred, const float* gt, int n, int K, int Tf, float scale, double* nll, void* stream) {
    if (stt_kde_check("sttode_kde_nll", pred, gt, n, K, Tf, nll)) return 1;
    hipLaunchKernelGGL(kde_nll_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, pred, gt, n, K, Tf, scale, nll);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_sample_spread(const float* pred, const float* gt, int n, int K, int Tf, float scale, double div_scale, double* apd,
                                    double* fpd, double* pade, double* dlow, double* es_ade, double* es_fde, float* ade_at_k, float* fde_at_k,
                                    void* stream) {
    if (stt_spread_check("sttode_sample_spread", pred, gt, n, K, Tf, div_scale, apd, fpd, pade, dlow, es_ade, es_fde, ade_at_k, fde_at_k))
        return 1;
    if (K <= SET_K1)
        hipLaunchKernelGGL((sample_spread_kernel<1, SET_K1>), dim3(n), dim3(256), 0, (hipStream_t)stream, pred, gt, K, Tf, scale, div_scale, apd,
                           fpd, pade, dlow, es_ade, es_fde, ade_at_k, fde_at_k);
    else
        hipLaunchKernelGGL((sample_spread_kernel<8, 64>), dim3(n), dim3(256), 0, (hipStream_t)stream, pred, gt, K, Tf, scale, div_scale, apd, fpd,
                           pade, dlow, es_ade, es_fde, ade_at_k, fde_at_k);
    STT_HIP(hipGetLastError());
    return 0;
}
