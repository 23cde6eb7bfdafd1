// Scene-level (joint) forms of the stage-2 objective's sample terms (include/sttode_hip.h sttode_sampler_objective_joint):
// the DLow kernel on the segment's mean squared distance, the reconstruction term with ONE best sample per segment, and the energy score
// on the scene's RMS displacement; kld stays per agent.  A segment (a scene, an NBA game) may hold hundreds of agents, so nothing stages
// a segment: the work goes in phases through a caller-provided workspace, each phase a launch of its own on the caller's stream.
//   sj_agent_kernel    (A) one wave per agent, sampler_objective_kernel's staging and pair-to-lane assignment.  kld[a] (sampler_body.hpp's
//                      sampler_kld, as sampler_loss_kernel: the same bits), and into the workspace the agent's np unmasked pair sums (float32, the DLow s), its np
//                      masked pair sums and its K per-sample sums against the ground truth (float64).
//   sj_segment_kernel  (B) one workgroup of 256 threads per segment.  Pairs and samples strided over the threads; each summed over the
//                      segment's agents in agent order in float64; a fixed-order LDS tree adds the threads; wave 0 runs the (value, index)
//                      butterfly.  -> div, rec, best, es [S] and the segment's coefficient tables exp(-d2_g / scale) [np], R_g(x_i, x_j) [np],
//                      R_g(x_k, y) [K] in the workspace.
//   sj_bwd_kernel      (C) one workgroup per agent, sampler_loss_bwd_kernel's (sample i, coordinate d) threads and its loop over j.  Reads
//                      its segment's tables (staged in LDS) and writes every element of dmotion, and dmu / dlogvar as sampler_loss_bwd_kernel.
// The forward entry runs A, B; the backward entry runs A, B (no outputs, tables only), C: it depends on nothing an earlier call left in
// the workspace.  A phase reads only what an EARLIER launch wrote.  No atomics, no flags; every sum's order is a function of the
// segment's size alone, so two runs give equal bits and a segment's outputs depend neither on the other segments nor on its place.
// Precision: kld, the per-agent DLow sums and the kld gradients float32 as sampler.hip; everything else float64; outputs float32.
#include <climits>
#include <cmath>

#include "api_util.hpp"
#include "sampler_body.hpp"

constexpr int SJ_LDS = 4096;   // floats of motion one agent may stage (K D), as sampler_loss_kernel
constexpr int SJ_WG = 256;     // threads of a segment's (B) and of an agent's backward (C) workgroup
static inline unsigned sj_lds_bytes(int K, int D) { return 4u * (unsigned)(K * D + D + D / 2); }
// (C) stages the segment's tables in front of the agent's samples: w [np] | 1/Rp [np] | 1/Rg [K] doubles
static inline unsigned sj_bwd_lds_bytes(int K, int D) { return 8u * (unsigned)(K * (K - 1) + K) + sj_lds_bytes(K, D); }   // 49 536 at most

// Workspace: per-agent doubles gs [n][K] | pm [n][np], per-segment doubles tw [S][np] | trp [S][np] | trg [S][K], then floats ps [n][np]
// and ints tbest [S].
struct SjWs {
    double *gs, *pm, *tw, *trp, *trg;
    float* ps;
    int* tbest;
};
static inline long sj_ws_bytes(long n, long K, long S) {
    const long np = K * (K - 1) / 2;
    return 8 * (n * K + n * np + 2 * S * np + S * K) + 4 * n * np + 4 * S;
}
static inline SjWs sj_ws_layout(void* ws, long n, long K, long S) {
    const long np = K * (K - 1) / 2;
    SjWs w;
    w.gs = (double*)ws;
    w.pm = w.gs + n * K;
    w.tw = w.pm + n * np;
    w.trp = w.tw + S * np;
    w.trg = w.trp + S * np;
    w.ps = (float*)(w.trg + S * K);
    w.tbest = (int*)(w.ps + n * np);
    return w;
}

// (A) one wave per agent
__global__ __launch_bounds__(64) void sj_agent_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                                                      const float* __restrict__ pmu, const float* __restrict__ plogvar,
                                                      const float* __restrict__ motion, const float* __restrict__ gt,
                                                      const float* __restrict__ mask, int n, int K, int nz, int D, float* __restrict__ kld,
                                                      float* __restrict__ ps, double* __restrict__ pm, double* __restrict__ gs) {
    extern __shared__ float sj_lds[];   // sM [K][D] | sY [D] | sW [Tf]: sj_lds_bytes(K, D), at most 28 KiB
    float *sM = sj_lds, *sY = sM + K * D, *sW = sY + D;
    const int a = blockIdx.x, lane = threadIdx.x;
    const int Tf = D / 2;
    if (kld) {   // (the backward's pass has no kld to write)
        const float kl = sampler_kld(mu, logvar, pmu, plogvar, a, K, nz, lane);
        if (lane == 0) kld[a] = kl;
    }
    sampler_stage(motion, gt, mask, a, K, D, lane, 64, sM, sY, sW);
    // pairs (i < j) in F.pdist order, pair p on lane p mod 64; s takes x then y of every frame in frame order, as sampler_loss_kernel
    const int np = K * (K - 1) / 2;
    for (int p = lane; p < np; p += 64) {
        int i, j;
        pdist_pair(p, K, i, j);
        float s = 0.f;
        double sm = 0.0;
        for (int t = 0; t < Tf; ++t) {
            const float xi = sM[i * D + 2 * t], xj = sM[j * D + 2 * t], yi = sM[i * D + 2 * t + 1], yj = sM[j * D + 2 * t + 1];
            const float dx = xi - xj;
            s = fmaf(dx, dx, s);
            const float dy = yi - yj;
            s = fmaf(dy, dy, s);
            const double m = (double)sW[t];
            const double ex = m * ((double)xi - (double)xj), ey = m * ((double)yi - (double)yj);
            sm += ex * ex + ey * ey;
        }
        ps[(size_t)a * np + p] = s;
        pm[(size_t)a * np + p] = sm;
    }
    // sample k on lane k mod 64: sum_t (m_t (x_k,t - y_t))^2 (the displacement sums are not wanted here)
    for (int k = lane; k < K; k += 64) {
        double ga = 0.0, last = 0.0;
        gs[(size_t)a * K + k] = sampler_gt_sample(sM, sY, sW, k, D, ga, last);
    }
}

// (B) one workgroup per segment.  div / rec / best / es may be NULL (the backward's pass): then only the tables are written.
__global__ __launch_bounds__(SJ_WG) void sj_segment_kernel(const int* __restrict__ seg_ptr, int n, int K, int D, float scale,
                                                           const float* __restrict__ ps, const double* __restrict__ pm,
                                                           const double* __restrict__ gs, double* __restrict__ tw, double* __restrict__ trp,
                                                           double* __restrict__ trg, int* __restrict__ tbest, float* __restrict__ div,
                                                           float* __restrict__ rec, int* __restrict__ best, float* __restrict__ es) {
    __shared__ double red[SJ_WG];
    __shared__ double sbv[SJ_WG];
    __shared__ int sbi[SJ_WG];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int np = K * (K - 1) / 2, Tf = D / 2;
    int a0, a1;
    clamped_segment(seg_ptr, g, n, a0, a1);
    const int ng = a1 - a0;
    if (ng <= 0) {   // an empty segment: NaN values, index 0 (no agent reads its tables)
        if (tid == 0) {
            tbest[g] = 0;
            if (div) {
                div[g] = NAN;
                rec[g] = NAN;
                best[g] = 0;
                es[g] = NAN;
            }
        }
        return;
    }
    const double inv_ng = 1.0 / (double)ng, inv_nt = 1.0 / ((double)ng * (double)Tf);
    double dsum = 0.0, rpsum = 0.0, rgsum = 0.0;
    for (int p = tid; p < np; p += SJ_WG) {
        double d2 = 0.0, m2 = 0.0;
        for (int a = a0; a < a1; ++a) {   // agent order
            d2 += (double)ps[(size_t)a * np + p];
            m2 += pm[(size_t)a * np + p];
        }
        const double w = exp(-(d2 * inv_ng) / (double)scale), rp = sqrt(m2 * inv_nt);
        tw[(size_t)g * np + p] = w;
        trp[(size_t)g * np + p] = rp;
        dsum += w;
        rpsum += rp;
    }
    double bv = INFINITY;
    int bi = INT_MAX;
    for (int k = tid; k < K; k += SJ_WG) {
        double J = 0.0;
        for (int a = a0; a < a1; ++a) J += gs[(size_t)a * K + k];
        const double rg = sqrt(J * inv_nt);
        trg[(size_t)g * K + k] = rg;
        rgsum += rg;
        if (J < bv) {   // (k ascending within a thread: the first minimum)
            bv = J;
            bi = k;
        }
    }
    dsum = index_tree_block_sum(dsum, red, tid);
    rpsum = index_tree_block_sum(rpsum, red, tid);
    rgsum = index_tree_block_sum(rgsum, red, tid);
    sbv[tid] = bv;
    sbi[tid] = bi;
    __syncthreads();
    if (tid < 64) {   // wave 0: the four waves' candidates of this lane, then the butterfly
        for (int q = 1; q < SJ_WG / 64; ++q) take_lower(bv, bi, sbv[tid + 64 * q], sbi[tid + 64 * q]);
        wave_take_lower(bv, bi);
        if (bi >= K) {   // no sample compared below +inf (NaN inputs)
            bi = 0;
            bv = NAN;
        }
        if (tid == 0) {
            tbest[g] = bi;
            if (div) {
                const double k1 = 1.0 / (double)K;
                div[g] = (float)(dsum / (double)np);
                rec[g] = (float)bv;
                best[g] = bi;
                es[g] = (float)(rgsum * k1 - rpsum * k1 * k1);
            }
        }
    }
}

// (C) one workgroup per agent
__global__ __launch_bounds__(SJ_WG) void sj_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                                                       const float* __restrict__ pmu, const float* __restrict__ plogvar,
                                                       const float* __restrict__ motion, const float* __restrict__ gt,
                                                       const float* __restrict__ mask, const int* __restrict__ seg_ptr, int S,
                                                       const float* __restrict__ g_kld, const float* __restrict__ g_div,
                                                       const float* __restrict__ g_rec, const float* __restrict__ g_es, int n, int K, int nz,
                                                       int D, float scale, const double* __restrict__ tw, const double* __restrict__ trp,
                                                       const double* __restrict__ trg, const int* __restrict__ tbest,
                                                       float* __restrict__ dmu, float* __restrict__ dlogvar, float* __restrict__ dmotion) {
    extern __shared__ double sj_lds_d[];   // sWt [np] | sIp [np] | sIg [K] doubles, then sM [K][D] | sY [D] | sW [Tf] floats: sj_bwd_lds_bytes
    const int np = K * (K - 1) / 2, Tf = D / 2;
    double *sWt = sj_lds_d, *sIp = sWt + np, *sIg = sIp + np;
    float *sM = (float*)(sIg + K), *sY = sM + K * D, *sW = sY + D;
    const int a = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)a * K * nz;
    const float gk = g_kld ? g_kld[a] : 0.f;
    for (int i = tid; i < K * nz; i += SJ_WG) {   // sampler_loss_bwd_kernel's statements
        const float ps = (plogvar ? expf(0.5f * plogvar[base + i]) : 1.f) + 1e-8f;
        const float t1 = (mu[base + i] - (pmu ? pmu[base + i] : 0.f)) / ps, t2 = expf(0.5f * logvar[base + i]) / ps;
        dmu[base + i] = gk * t1 / ps;
        dlogvar[base + i] = gk * 0.5f * (t2 * t2 - 1.0f);
    }
    // the agent's segment: the last g whose (clamped) start is <= a; an agent that no segment holds gets a zero gradient
    int lo = 0, hi = S - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (min(max(seg_ptr[mid], 0), n) <= a) lo = mid;
        else hi = mid - 1;
    }
    const int g = lo;
    int a0, a1;
    clamped_segment(seg_ptr, g, n, a0, a1);
    if (a < a0 || a >= a1) {
        for (int e = tid; e < K * D; e += SJ_WG) dmotion[(size_t)a * K * D + e] = 0.f;
        return;
    }
    const int ng = a1 - a0;
    for (int i = tid; i < np; i += SJ_WG) {
        sWt[i] = tw[(size_t)g * np + i];
        const double r = trp[(size_t)g * np + i];
        sIp[i] = r > 0.0 ? 1.0 / r : 0.0;   // R = 0: no gradient (the subgradient 0 of a norm at 0)
    }
    for (int i = tid; i < K; i += SJ_WG) {
        const double r = trg[(size_t)g * K + i];
        sIg[i] = r > 0.0 ? 1.0 / r : 0.0;
    }
    sampler_stage(motion, gt, mask, a, K, D, tid, SJ_WG, sM, sY, sW);
    const int bi = tbest[g];
    const double gd = g_div ? (double)g_div[g] : 0.0, gr = g_rec ? (double)g_rec[g] : 0.0, ge = g_es ? (double)g_es[g] : 0.0;
    const double cd = gd * (-2.0 / ((double)scale * (double)ng)) / (double)np;
    const double k1 = 1.0 / (double)K;
    const double ce = ge / ((double)ng * (double)Tf);
    // thread = (sample i, coordinate d), frame t = d / 2, j in ascending order:
    //   DLow    cd * sum_{j != i} w_ij (x_i - x_j)
    //   energy  ce * ( m (m (x_i - y)) / (K Rg_i) - sum_{j != i} m (m (x_i - x_j)) / (K^2 Rp_ij) )
    //   rec     g_rec * 2 m (m (x_i - y)) for i == best
    for (int e = tid; e < K * D; e += SJ_WG) {
        const int i = e / D, d = e % D;
        const double m = (double)sW[d / 2], xi = (double)sM[e];
        double acc = 0.0, us = 0.0;
        for (int j = 0; j < K; ++j) {
            if (j == i) continue;
            const int lo_ = i < j ? i : j, hi_ = i < j ? j : i;
            const int p = lo_ * (2 * K - lo_ - 1) / 2 + (hi_ - lo_ - 1);
            const double df = xi - (double)sM[j * D + d];
            acc += sWt[p] * df;
            us += df * sIp[p];
        }
        const double ec = m * (m * (xi - (double)sY[d]));
        double v = cd * acc + ce * (ec * sIg[i] * k1 - m * m * us * k1 * k1);
        if (i == bi) v += gr * 2.0 * ec;
        dmotion[(size_t)a * K * D + e] = (float)v;
    }
}

static int sj_check(const char* who, const void* mu, const void* logvar, const void* motion, const void* gt, const void* seg_ptr,
                    const void* workspace, bool outs, int S, int n, int K, int nz, int D, float scale, long ws_bytes) {
    const char* why = nullptr;
    if (!(mu && logvar && motion && gt && seg_ptr && workspace && outs))
        why = "null pointer (mu, logvar, motion, gt, seg_ptr, workspace and every output are required)";
    else if (!(n > 0 && nz > 0 && D > 0)) why = "n, nz, D must be positive";
    else if (K <= 1) why = "K must be > 1";
    else if (S < 1) why = "S must be >= 1";
    else if (D % 2 != 0) why = "D must be even (D = 2 Tf)";
    else if ((long)K * D > SJ_LDS) why = "K * D must be <= 4096";
    else if (!(scale > 0.f)) why = "scale must be positive";
    else if (((size_t)workspace & 7) != 0) why = "workspace must be aligned to 8 bytes";
    else if (ws_bytes < sj_ws_bytes(n, K, S)) why = "ws_bytes is less than sttode_sampler_objective_joint_ws(n, K, S)";
    return why ? stt_refuse(who, why) : 0;
}

extern "C" long long int sttode_sampler_objective_joint_ws(int n, int K, int S) {
    if (n <= 0 || K <= 1 || S < 1 || K > SJ_LDS / 2) {
        stt_set_error("sttode_sampler_objective_joint_ws: n > 0, 1 < K <= 2048 and S >= 1 expected");
        return -1;
    }
    return (long long)sj_ws_bytes(n, K, S);
}

// phases A and B on `stream`
static int sj_forward(const float* mu, const float* logvar, const float* pmu, const float* plogvar, const float* motion, const float* gt,
                      const float* mask, const int* seg_ptr, int S, int n, int K, int nz, int D, float scale, const SjWs& w, float* kld,
                      float* div, float* rec, int* best, float* es, hipStream_t stream) {
    hipLaunchKernelGGL(sj_agent_kernel, dim3(n), dim3(64), sj_lds_bytes(K, D), stream, mu, logvar, pmu, plogvar, motion, gt, mask, n, K, nz, D,
                       kld, w.ps, w.pm, w.gs);
    STT_HIP(hipGetLastError());
    hipLaunchKernelGGL(sj_segment_kernel, dim3(S), dim3(SJ_WG), 0, stream, seg_ptr, n, K, D, scale, w.ps, w.pm, w.gs, w.tw, w.trp, w.trg,
                       w.tbest, div, rec, best, es);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_sampler_objective_joint(const float* mu, const float* logvar, const float* pmu, const float* plogvar,
                                              const float* motion, const float* gt, const float* mask, const int* seg_ptr, int S, int n, int K,
                                              int nz, int D, float scale, void* workspace, long ws_bytes, float* kld, float* div,
                                              float* rec, int* best, float* es, void* stream) {
    if (sj_check("sttode_sampler_objective_joint", mu, logvar, motion, gt, seg_ptr, workspace, kld && div && rec && best && es, S, n, K, nz, D,
                 scale, ws_bytes))
        return 1;
    return sj_forward(mu, logvar, pmu, plogvar, motion, gt, mask, seg_ptr, S, n, K, nz, D, scale, sj_ws_layout(workspace, n, K, S), kld, div,
                      rec, best, es, (hipStream_t)stream);
}

extern "C" int sttode_sampler_objective_joint_bwd(const float* mu, const float* logvar, const float* pmu, const float* plogvar,
                                                  const float* motion, const float* gt, const float* mask, const int* seg_ptr, int S,
                                                  const float* g_kld, const float* g_div, const float* g_rec, const float* g_es, int n, int K,
                                                  int nz, int D, float scale, void* workspace, long ws_bytes, float* dmu, float* dlogvar,
                                                  float* dmotion, void* stream) {
    if (sj_check("sttode_sampler_objective_joint_bwd", mu, logvar, motion, gt, seg_ptr, workspace, dmu && dlogvar && dmotion, S, n, K, nz, D,
                 scale, ws_bytes))
        return 1;
    const SjWs w = sj_ws_layout(workspace, n, K, S);
    // the segment tables are recomputed here (A, B without outputs): the call does not rely on what an earlier one left in the workspace
    if (int rc = sj_forward(mu, logvar, pmu, plogvar, motion, gt, mask, seg_ptr, S, n, K, nz, D, scale, w, nullptr, nullptr, nullptr, nullptr,
                            nullptr, (hipStream_t)stream))
        return rc;
    hipLaunchKernelGGL(sj_bwd_kernel, dim3(n), dim3(SJ_WG), sj_bwd_lds_bytes(K, D), (hipStream_t)stream, mu, logvar, pmu, plogvar, motion, gt,
                       mask, seg_ptr, S, g_kld, g_div, g_rec, g_es, n, K, nz, D, scale, w.tw, w.trp, w.trg, w.tbest, dmu, dlogvar, dmotion);
    STT_HIP(hipGetLastError());
    return 0;
}
