// A weighted sample set scored against the ground truth (include/sttode_hip.h sttode_weighted_set): K representatives per agent
// with raw weights w_k (cluster counts or probabilities, sttode_reduce_samples' `counts` / M), p_k = w_k / sum w.  Expected ADE / FDE, the
// energy scores and the expected pairwise distances under p, the KDE NLL of scipy.stats.gaussian_kde(weights=), the probability-ranked
// best-of-k rows, the Brier-penalised minimum and the effective sample size, in one launch.  The reference computes none of them.
//   weighted_set_kernel  one workgroup of 256 threads per agent, the layout of sample_spread_kernel (the tile pieces of set_body.hpp): raw float2 samples through
//                        LDS in tiles of SET_FT frames with an odd row stride; the pairs in F.pdist order on threads p mod 256; wave 2 with
//                        lane = sample for the distances to the ground truth and the rank; wave 3 with lane = frame for the KDE frames.
// No atomics: every sum has a fixed order, so two runs give the same bits and an agent's values do not depend on the rest of the batch.
#include <cmath>

#include "api_util.hpp"
#include "set_body.hpp"
#include "../../include/sttode_hip.h"

namespace {

// Lane q's value of v in every lane; q must be the same in all lanes.
__device__ __forceinline__ double lane_value(double v, int q) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), q), __builtin_amdgcn_readlane(__double2loint(v), q));
}

// Agent a = blockIdx.x.  Coordinates are (double)(x * scale) with the product in fp32; everything after that is float64 but ADE_k / FDE_k,
// which are bok_select_kernel's fp32 values (bok_dist, frames in frame order).
// Weights (wave 0, lane = sample): W = sum of w_k in sample order, p_k = w_k / W, s2 = sum of p_k^2 in sample order, every lane forming the
// same sums from LDS.  A negative or non-finite weight or W == 0 marks the row bad: all its outputs are NaN.  Multiplying every weight by a
// power of two changes no bit (the quotients are the same).
// Pairs: pair q (F.pdist order) belongs to thread q mod 256; a pair with p_i p_j == 0 is dropped before any of its coordinates is read.  Per
// pair the running sum of squared distances, of distances and the last frame's distance, frames in frame order; after the last tile the
// thread adds p_i p_j times (mean distance, last distance, root of the summed squares) over its pairs in pair order; the three partials go
// through LDS, wave 0 adds lane l, l + 64, l + 128, l + 192 in that order and the 64 lanes by a fixed xor tree.
// Wave 2, lane = sample k with w_k > 0 (the others read nothing): float64 mean / last distance to the ground truth D_k / L_k, and ADE_k / FDE_k
// in fp32.  p_k D_k and p_k L_k over the lanes by the xor tree.  rank_k = #{j : w_j > w_k or (w_j == w_k and j < k)} by counting over the raw
// weights in LDS; ADE_k / FDE_k scattered to slot rank_k (zero-weight samples: +inf, they rank last), an inclusive prefix fminf over the slots
// (NaN skipped, the idle lanes' +inf as sample_spread_kernel) gives the *_top rows.  k* = the lowest k with w_k > 0 whose ADE_k equals the
// minimum (a ballot); brier = (double)min + (1 - p_k*)^2; FDE alike.
// Wave 3, lane = frame of the tile (needs P >= 3 positive weights and 1 - s2 > 0): over the samples with w_k > 0 in sample order the mean
// m = sum p_k x_k, C = sum p_k (x_k - m)(x_k - m)^T / (1 - s2), Sigma = f^2 C with f = neff^(-1/6) = s2^(1/6), logsumexp_k(log p_k - q_k / 2) in
// two passes (max, then the sum of exp), minus log det(2 pi Sigma) / 2, clipped below at -20; the tile's frames by the xor tree, tiles in
// order; nll = -sum / Tf.  C00 <= 0 or det C <= 0 at some frame: NaN (kde_nll_kernel's rule).  The positive-weight samples (k, p_k, log p_k)
// are compacted by wave 0 and kept by wave 3 in registers, entry q in lane q, read by v_readlane inside the loops over q.
// R = pairs per thread, KM = the largest K, as sample_spread_kernel: <8, 64> takes any K, <1, SET_K1> is the same code for K <= 23.
// The workgroup waits on its KDE wave, so the time of a launch is set by how many workgroups a CU holds: <1, SET_K1> is built for 6 waves
// per SIMD (80 VGPRs, 68 bytes of scratch per lane; measured against 4 waves without scratch and 8 with 136 bytes: DESIGN.md 7).
template <int R, int KM>
__global__ __launch_bounds__(256, R == 1 ? 6 : 2) void weighted_set_kernel(const float* __restrict__ pred, const float* __restrict__ weights,
                                                           const float* __restrict__ gt, int K, int Tf, float scale, double* __restrict__ eade,
                                                           double* __restrict__ efde, double* __restrict__ es_ade, double* __restrict__ es_fde,
                                                           double* __restrict__ apd, double* __restrict__ fpd, double* __restrict__ kde,
                                                           double* __restrict__ brier_ade, double* __restrict__ brier_fde,
                                                           double* __restrict__ neff, float* __restrict__ ade_top, float* __restrict__ fde_top) {
    __shared__ float2 sx[KM * SET_STRIDE];
    __shared__ float2 sg[SET_FT];
    __shared__ double red[3][256];
    __shared__ double sp[64];                    // p_k (0 beyond K)
    __shared__ double cp[64], clp[64];           // the samples with w_k > 0, compacted in sample order: p_k and log p_k
    __shared__ int cix[64];                      // ... and their k
    __shared__ double sc[8];                     // s2 | E ade | E fde | kde | brier ade | brier fde
    __shared__ float sw[64], sa[64], sf[64];     // raw weights (0 beyond K); ADE / FDE by rank
    __shared__ int sflag[2];                     // bad row | positive weights
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int a = blockIdx.x;
    const int P = K * (K - 1) / 2;
    const float2* p = reinterpret_cast<const float2*>(pred + (size_t)a * K * Tf * 2);
    const float2* g = reinterpret_cast<const float2*>(gt + (size_t)a * Tf * 2);
    if (w == 0) {
        const float wk = lane < K ? weights[(size_t)a * K + lane] : 0.f;
        sw[lane] = wk;
        const bool neg = wk < 0.f || !(fabsf(wk) <= 3.402823466e38f);
        const unsigned long long posm = __ballot(wk > 0.f);
        const int npos = __popcll(posm);
        __builtin_amdgcn_wave_barrier();
        double W = 0.0;
        for (int k = 0; k < K; ++k) W += (double)sw[k];
        const bool bad = __ballot(neg) != 0 || !(W > 0.0);
        const double pk = lane < K ? (double)wk / W : 0.0;
        sp[lane] = pk;
        if (wk > 0.f) {
            const int q = __popcll(posm & ((1ull << lane) - 1ull));
            cp[q] = pk;
            clp[q] = log(pk);
            cix[q] = lane;
        }
        __builtin_amdgcn_wave_barrier();
        double s2 = 0.0;
        for (int k = 0; k < K; ++k) s2 += sp[k] * sp[k];
        if (lane == 0) {
            sc[0] = s2;
            sflag[0] = bad;
            sflag[1] = npos;
        }
    }
    int ij[R];                                   // (i, j) of the thread's r-th pair as i | j << 8
    double s2[R], s1[R], dl[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int q = tid + 256 * r, i = 0;
        if (q < P) i = pdist_row(q, K);
        ij[r] = i | (i + 1 + q) << 8;
        s2[r] = s1[r] = dl[r] = 0.0;
    }
    __syncthreads();
    unsigned live = 0;                           // bit r: the r-th pair has p_i p_j != 0
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (tid + 256 * r < P && sp[ij[r] & 255] * sp[ij[r] >> 8] != 0.0) live |= 1u << r;
    const bool bad_row = sflag[0] != 0;
    const float wk = sw[lane];
    const bool gw = w == 2 && wk > 0.f;                                      // wave 2, lane = a sample of the set
    const int npos = __builtin_amdgcn_readfirstlane(sflag[1]);
    const bool kw = w == 3 && kde != nullptr && npos >= 3 && 1.0 - sc[0] > 0.0 && !bad_row;   // wave 3 runs the KDE frames
    const double om = 1.0 - sc[0], f2 = cbrt(sc[0]);                         // f^2 = neff^(-1/3)
    double ga = 0.0, gl = 0.0;                   // wave 2: sum over frames of |x_k - y| and the last frame's, float64
    float fa = 0.f, fl = 0.f;                    // the same with bok_dist in fp32
    double acc = 0.0;                            // wave 3: sum of the clipped log-densities
    bool sing = false;
    // wave 3 keeps the compacted samples in registers, entry q in lane q: a loop over q reads them by v_readlane (q is uniform), so that no
    // LDS address of its loops waits on an LDS read
    const int rix = cix[lane] * SET_STRIDE;
    const double rp = cp[lane], rlp = clp[lane];
    for (int t0 = 0; t0 < Tf; t0 += SET_FT) {
        const int ft = min(SET_FT, Tf - t0);
        stage_tile<size_t>(sx, sg, p, g, K, Tf, t0, ft, tid);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (live >> r & 1) pair_tile_accumulate(sx, ij[r], ft, scale, s2[r], s1[r], dl[r]);
        if (gw) gt_tile_accumulate(sx, sg, lane, ft, scale, ga, gl, fa, fl);
        if (kw) {
            // every lane runs every loop (the lane reads need all lanes active); a lane beyond the tile redoes its last frame and drops the
            // value, as a lane whose frame is singular does
            const int tl = min(lane, ft - 1);
            double mx = 0.0, my = 0.0;
            for (int q = 0; q < npos; ++q) {
                const float2 v = sx[__builtin_amdgcn_readlane(rix, q) + tl];
                const double pq = lane_value(rp, q);
                mx += pq * (double)(v.x * scale);
                my += pq * (double)(v.y * scale);
            }
            double c00 = 0.0, c01 = 0.0, c11 = 0.0;
            for (int q = 0; q < npos; ++q) {
                const float2 v = sx[__builtin_amdgcn_readlane(rix, q) + tl];
                const double dx = (double)(v.x * scale) - mx, dy = (double)(v.y * scale) - my;
                const double pq = lane_value(rp, q);
                c00 += pq * (dx * dx);
                c01 += pq * (dx * dy);
                c11 += pq * (dy * dy);
            }
            c00 /= om;
            c01 /= om;
            c11 /= om;
            const float2 y = sg[tl];
            const double gx = (double)(y.x * scale), gy = (double)(y.y * scale);
            double det, inv;
            const bool pd = kde_cov(c00, c01, c11, f2, det, inv);
            double m = -INFINITY;
            for (int q = 0; q < npos; ++q) {
                const float2 v = sx[__builtin_amdgcn_readlane(rix, q) + tl];
                const double dx = gx - (double)(v.x * scale), dy = gy - (double)(v.y * scale);
                m = fmax(m, lane_value(rlp, q) - 0.5 * kde_quad(c00, c01, c11, inv, dx, dy));
            }
            double sum = 0.0;
            for (int q = 0; q < npos; ++q) {
                const float2 v = sx[__builtin_amdgcn_readlane(rix, q) + tl];
                const double dx = gx - (double)(v.x * scale), dy = gy - (double)(v.y * scale);
                sum += exp(lane_value(rlp, q) - 0.5 * kde_quad(c00, c01, c11, inv, dx, dy) - m);
            }
            const double lp = kde_clip(log(sum) + m - kde_log_norm(f2, det));
            sing |= lane < ft && !pd;
            acc += wave_sum(lane < ft && pd ? lp : 0.0);
        }
        __syncthreads();   // (the next tile overwrites sx and sg)
    }
    double t_a = 0.0, t_f = 0.0, t_t = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (live >> r & 1) {
            const double pp = sp[ij[r] & 255] * sp[ij[r] >> 8];
            t_a += pp * (s1[r] / Tf);
            t_f += pp * dl[r];
            t_t += pp * sqrt(s2[r]);
        }
    }
    red[0][tid] = t_a;
    red[1][tid] = t_f;
    red[2][tid] = t_t;
    if (w == 2) {
        const double pk = sp[lane];
        const double da = wave_sum(gw ? pk * (ga / Tf) : 0.0), df = wave_sum(gw ? pk * gl : 0.0);
        if (lane == 0) {
            sc[1] = da;
            sc[2] = df;
        }
        const float ka = gw ? fa / (float)Tf : INFINITY, kf = gw ? fl : INFINITY;   // ADE_k / FDE_k of the lane's sample
        int rank = 0;
        for (int j = 0; j < K; ++j) {
            const float wj = sw[j];
            rank += (wj > wk || (wj == wk && j < lane)) ? 1 : 0;
        }
        sa[lane] = INFINITY;
        sf[lane] = INFINITY;
        __builtin_amdgcn_wave_barrier();
        if (lane < K) {                          // (a bad row's ranks may collide; they stay below K)
            sa[rank] = ka;
            sf[rank] = kf;
        }
        __builtin_amdgcn_wave_barrier();
        const float va = prefix_fmin64(sa[lane], lane), vf = prefix_fmin64(sf[lane], lane);
        if (lane < K) {
            if (ade_top) ade_top[(size_t)a * K + lane] = bad_row ? NAN : va;
            if (fde_top) fde_top[(size_t)a * K + lane] = bad_row ? NAN : vf;
        }
        const float ma = __shfl(va, 63, 64), mf = __shfl(vf, 63, 64);   // the minimum over the whole set
        const unsigned long long ba = __ballot(gw && ka == ma), bf = __ballot(gw && kf == mf);
        if (lane == 0) {
            const double qa = ba ? 1.0 - sp[__ffsll((long long)ba) - 1] : (double)NAN;
            const double qf = bf ? 1.0 - sp[__ffsll((long long)bf) - 1] : (double)NAN;
            sc[4] = (double)ma + qa * qa;
            sc[5] = (double)mf + qf * qf;
        }
    }
    if (w == 3) {
        const bool any_sing = __ballot(sing) != 0;
        if (lane == 0) sc[3] = kw && !any_sing ? -acc / Tf : (double)NAN;
    }
    __syncthreads();
    if (w != 0) return;
    double v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {   // (quad_then_wave_sum's order, spelled out: through the helper the <1, 23> form's scratch size moves)
        v[q] = ((red[q][lane] + red[q][lane + 64]) + red[q][lane + 128]) + red[q][lane + 192];
        v[q] = wave_sum(v[q]);
    }
    if (lane == 0) {
        const double nan = (double)NAN;
        const bool one = !(om > 0.0);            // a single positive weight: no two different draws
        eade[a] = bad_row ? nan : sc[1];
        efde[a] = bad_row ? nan : sc[2];
        es_ade[a] = bad_row ? nan : sc[1] - v[0];
        es_fde[a] = bad_row ? nan : sc[2] - v[1];
        apd[a] = bad_row || one ? nan : 2.0 * v[2] / om;
        fpd[a] = bad_row || one ? nan : 2.0 * v[1] / om;
        neff[a] = bad_row ? nan : 1.0 / sc[0];
        if (kde) kde[a] = sc[3];
        if (brier_ade) brier_ade[a] = bad_row ? nan : sc[4];
        if (brier_fde) brier_fde[a] = bad_row ? nan : sc[5];
    }
}

}  // namespace

// Argument checks: 0, or 1 with the error set naming `who`.
static int weighted_check(const char* who, const float* pred, const float* weights, const float* gt, int n, int K, int Tf, const double* eade,
                          const double* efde, const double* es_ade, const double* es_fde, const double* apd, const double* fpd,
                          const double* neff) {
    const char* why = nullptr;
    if (!(pred && weights && gt))
        why = "null pointer (pred, weights and gt are required)";
    else if (!(eade && efde && es_ade && es_fde && apd && fpd && neff))
        why = "null pointer (eade, efde, es_ade, es_fde, apd, fpd and neff are required)";
    else if (!(n > 0 && Tf > 0))
        why = "n and Tf must be positive";
    else if (K < 1 || K > 64)
        why = "needs 1 <= K <= 64 (one lane per sample)";
    return why ? stt_refuse(who, why) : 0;
}

extern "C" int sttode_weighted_set(const float* pred, const float* weights, const float* gt, int n, int K, int Tf, float scale, double* eade,
                                   double* efde, double* es_ade, double* es_fde, double* apd, double* fpd, double* kde_nll, double* brier_ade,
                                   double* brier_fde, double* neff, float* ade_top, float* fde_top, void* stream) {
    if (weighted_check("sttode_weighted_set", pred, weights, gt, n, K, Tf, eade, efde, es_ade, es_fde, apd, fpd, neff)) return 1;
    if (K <= SET_K1)
        hipLaunchKernelGGL((weighted_set_kernel<1, SET_K1>), dim3(n), dim3(256), 0, (hipStream_t)stream, pred, weights, gt, K, Tf, scale, eade,
                           efde, es_ade, es_fde, apd, fpd, kde_nll, brier_ade, brier_fde, neff, ade_top, fde_top);
    else
        hipLaunchKernelGGL((weighted_set_kernel<8, 64>), dim3(n), dim3(256), 0, (hipStream_t)stream, pred, weights, gt, K, Tf, scale, eade, efde,
                           es_ade, es_fde, apd, fpd, kde_nll, brier_ade, brier_fde, neff, ade_top, fde_top);
    STT_HIP(hipGetLastError());
    return 0;
}
