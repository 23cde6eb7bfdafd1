// Stage-2 objective with its ground-truth terms (include/sttode_hip.h sttode_sampler_objective): next to sampler.hip's
// kld / div, the reconstruction term of samplerloss.py:23-29 (min over K of the masked squared error) and the energy scores of 4s, in one
// launch over all agents, and their backward in a second one.
//   sampler_objective_kernel      one wave per agent.  kld is sampler_body.hpp's sampler_kld and div has sampler_loss_kernel's statements, lane for lane and in its
//                                 order (the same bits); the loop over the pairs that forms dx, dy for sum d^2 also takes the per-frame
//                                 norm |x_i,t - x_j,t| for pade / fpd.  Lane k then walks sample k against the ground truth.
//   sampler_objective_bwd_kernel  sampler_loss_bwd_kernel's (sample i, coordinate d) threads; inside its loop over j the frame's unit
//                                 vector joins the DLow term, and the ground-truth half and the best sample's 2 m^2 (x - y) are added.
// Precision: kld, div and their gradients float32 as in sampler.hip.  The new terms: differences to the ground truth, their norms and every
// sum in float64; the pair norms sqrtf of float32 dx, dy (the very registers of the DLow sum), summed in float64.  No atomics; pairs and
// samples are dealt to lanes by index and the 64 lanes added by a fixed xor tree: the same bits on every run.
// LDS is sized at the launch (so_lds_bytes: samples, ground truth, mask; 2 064 bytes at K = 20, Tf = 12, 28 KiB at most), so that a CU holds
// as many one-wave workgroups as the shape allows: the kernels wait on LDS latency, not on arithmetic.
#include <climits>
#include <cmath>

#include "api_util.hpp"
#include "sampler_body.hpp"

constexpr int SO_LDS = 4096;   // floats of motion one agent may stage (K D), as sampler_loss_kernel
static inline unsigned so_lds_bytes(int K, int D) { return 4u * (unsigned)(K * D + D + D / 2); }   // K >= 2: at most 4 (4096 + 2048 + 1024)

// Ground-truth half.  Sample k belongs to lane k mod 64; per sample, frames in frame order, float64:
//   rec_k = sum_t (m_t (x_k,t - y_t))^2, and the displacements |m_t (x_k,t - y_t)| summed over the frames (ga) and at the last one (gl).
// -> the smallest rec_k and the smallest index that has it (every lane holds both); ga, gl summed over the lane's samples.
static __device__ inline void so_gt_half(const float* sM, const float* sY, const float* sW, int K, int D, int lane, double& rec, int& best,
                                         double& ga, double& gl) {
    double bv = INFINITY;
    int bi = INT_MAX;
    ga = gl = 0.0;
    for (int k = lane; k < K; k += 64) {
        double last = 0.0;
        const double r2 = sampler_gt_sample(sM, sY, sW, k, D, ga, last);
        gl += last;
        if (r2 < bv) {
            bv = r2;
            bi = k;
        }
    }
    wave_take_lower(bv, bi);
    if (bi >= K) {   // no sample compared below +inf (NaN inputs)
        bi = 0;
        bv = NAN;
    }
    rec = bv;
    best = bi;
}

__global__ __launch_bounds__(64) void sampler_objective_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                                                               const float* __restrict__ pmu, const float* __restrict__ plogvar,
                                                               const float* __restrict__ motion, const float* __restrict__ gt,
                                                               const float* __restrict__ mask, int n, int K, int nz, int D, float scale,
                                                               float* __restrict__ kld, float* __restrict__ div, float* __restrict__ rec,
                                                               int* __restrict__ best, float* __restrict__ es_ade,
                                                               float* __restrict__ es_fde) {
    extern __shared__ float so_lds[];   // sM [K][D] | sY [D] | sW [Tf]: so_lds_bytes(K, D), at most 28 KiB
    float *sM = so_lds, *sY = sM + K * D, *sW = sY + D;
    const int a = blockIdx.x, lane = threadIdx.x;
    const int Tf = D / 2;
    const float kl = sampler_kld(mu, logvar, pmu, plogvar, a, K, nz, lane);
    sampler_stage(motion, gt, mask, a, K, D, lane, 64, sM, sY, sW);
    // pairs (i < j) in F.pdist order, pair p on lane p mod 64 as in sampler_loss_kernel; s takes x then y of every frame, in frame order
    const int np = K * (K - 1) / 2;
    float acc = 0.f;
    double pa = 0.0, pf = 0.0;   // over the lane's pairs: the per-frame norms summed over the frames, and the last frame's
    for (int p = lane; p < np; p += 64) {
        int i, j;
        pdist_pair(p, K, i, j);
        float s = 0.f, last = 0.f;
        for (int t = 0; t < Tf; ++t) {
            // (fmaf spelled out: sampler_loss_kernel's `s += t * t` compiles to one fused multiply-add per coordinate, and the bits must agree)
            const float dx = sM[i * D + 2 * t] - sM[j * D + 2 * t];
            s = fmaf(dx, dx, s);
            const float dy = sM[i * D + 2 * t + 1] - sM[j * D + 2 * t + 1];
            s = fmaf(dy, dy, s);
            const float ex = sW[t] * dx, ey = sW[t] * dy;
            last = sqrtf(ex * ex + ey * ey);
            pa += (double)last;
        }
        pf += (double)last;
        const float dist = sqrtf(s);
        acc += expf(-(dist * dist) / scale);
    }
    acc = wave_sum(acc);
    pa = wave_sum(pa);
    pf = wave_sum(pf);
    double rv, ga, gl;
    int bi;
    so_gt_half(sM, sY, sW, K, D, lane, rv, bi, ga, gl);
    ga = wave_sum(ga);
    gl = wave_sum(gl);
    if (lane == 0) {
        kld[a] = kl;
        div[a] = acc / (float)np;
        rec[a] = (float)rv;
        best[a] = bi;
        // (1/K) sum_k D(x_k, y) - ((K-1)/(2K)) * (pair mean) = sum_k / K - (pair sum) / K^2
        const double k1 = 1.0 / (double)K, k2 = k1 * k1;
        es_ade[a] = (float)((ga * k1 - pa * k2) / (double)Tf);
        es_fde[a] = (float)(gl * k1 - pf * k2);
    }
}

__global__ __launch_bounds__(64) void sampler_objective_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                                                                   const float* __restrict__ pmu, const float* __restrict__ plogvar,
                                                                   const float* __restrict__ motion, const float* __restrict__ gt,
                                                                   const float* __restrict__ mask, const float* __restrict__ g_kld,
                                                                   const float* __restrict__ g_div, const float* __restrict__ g_rec,
                                                                   const float* __restrict__ g_es_ade, const float* __restrict__ g_es_fde,
                                                                   int n, int K, int nz, int D, float scale, float* __restrict__ dmu,
                                                                   float* __restrict__ dlogvar, float* __restrict__ dmotion) {
    extern __shared__ float so_lds[];   // sM [K][D] | sY [D] | sW [Tf]: so_lds_bytes(K, D), at most 28 KiB
    float *sM = so_lds, *sY = sM + K * D, *sW = sY + D;
    const int a = blockIdx.x, lane = threadIdx.x;
    const int Tf = D / 2;
    const size_t base = (size_t)a * K * nz;
    const float gk = g_kld ? g_kld[a] : 0.f, gd = g_div ? g_div[a] : 0.f;
    const double gr = g_rec ? (double)g_rec[a] : 0.0;
    const double gea = g_es_ade ? (double)g_es_ade[a] / (double)Tf : 0.0, gef = g_es_fde ? (double)g_es_fde[a] : 0.0;
    for (int i = lane; i < K * nz; i += 64) {
        const float ps = (plogvar ? expf(0.5f * plogvar[base + i]) : 1.f) + 1e-8f;
        const float t1 = (mu[base + i] - (pmu ? pmu[base + i] : 0.f)) / ps, t2 = expf(0.5f * logvar[base + i]) / ps;
        dmu[base + i] = gk * t1 / ps;
        dlogvar[base + i] = gk * 0.5f * (t2 * t2 - 1.0f);
    }
    sampler_stage(motion, gt, mask, a, K, D, lane, 64, sM, sY, sW);
    double rv, ga, gl;
    int bi;
    so_gt_half(sM, sY, sW, K, D, lane, rv, bi, ga, gl);   // the forward's choice of the best sample, by the forward's code
    const float coef = gd * (-2.0f / scale) / (float)(K * (K - 1) / 2);
    const double k1 = 1.0 / (double)K, k2 = k1 * k1;
    // thread = (sample i, coordinate d), frame t = d / 2:
    //   DLow    coef * sum_{j != i} exp(-|m_i - m_j|^2 / scale) (m_i - m_j)                      (sampler_loss_bwd_kernel, in its order)
    //   energy  ce_t * ( u(x_i,t - y_t) / K - sum_{j != i} u(x_i,t - x_j,t) / K^2 ),  u(v) = m_t (m_t v) / |m_t v|, 0 at v = 0,
    //           ce_t = g_es_ade / Tf + (t == Tf - 1) g_es_fde
    //   rec     g_rec * 2 m_t (m_t (x_i - y)) for i == best
    for (int e = lane; e < K * D; e += 64) {
        const int i = e / D, d = e % D, t = d / 2;
        const float w = sW[t];
        float acc = 0.f;
        double us = 0.0;
        for (int j = 0; j < K; ++j) {
            if (j == i) continue;
            float s = 0.f;
            for (int q = 0; q < D; ++q) {
                const float df = sM[i * D + q] - sM[j * D + q];
                s = fmaf(df, df, s);
            }
            if (s > 0.f) acc = fmaf(expf(-s / scale), sM[i * D + d] - sM[j * D + d], acc);   // F.pdist backward is 0 at zero distance
            const float ex = w * (sM[i * D + 2 * t] - sM[j * D + 2 * t]), ey = w * (sM[i * D + 2 * t + 1] - sM[j * D + 2 * t + 1]);
            const float r2 = ex * ex + ey * ey;
            if (r2 > 0.f) us += (double)(w * ((d & 1) ? ey : ex) / sqrtf(r2));
        }
        const double m = (double)w;
        const double ex = m * ((double)sM[i * D + 2 * t] - (double)sY[2 * t]), ey = m * ((double)sM[i * D + 2 * t + 1] - (double)sY[2 * t + 1]);
        const double ec = (d & 1) ? ey : ex, g2 = ex * ex + ey * ey;
        const double ug = g2 > 0.0 ? m * ec / sqrt(g2) : 0.0;
        const double ce = gea + (t == Tf - 1 ? gef : 0.0);
        double extra = ce * (ug * k1 - us * k2);
        if (i == bi) extra += gr * 2.0 * m * ec;
        dmotion[(size_t)a * K * D + e] = coef * acc + (float)extra;
    }
}

static int so_check(const char* who, const void* mu, const void* logvar, const void* motion, const void* gt, bool outs, int n, int K, int nz,
                    int D, float scale) {
    const char* why = nullptr;
    if (!(mu && logvar && motion && gt && outs)) why = "null pointer (mu, logvar, motion, gt and every output are required)";
    else if (!(n > 0 && nz > 0 && D > 0)) why = "n, nz, D must be positive";
    else if (K <= 1) why = "K must be > 1";
    else if (D % 2 != 0) why = "D must be even (D = 2 Tf)";
    else if ((long)K * D > SO_LDS) why = "K * D must be <= 4096";
    else if (!(scale > 0.f)) why = "scale must be positive";
    return why ? stt_refuse(who, why) : 0;
}

extern "C" int sttode_sampler_objective(const float* mu, const float* logvar, const float* pmu, const float* plogvar, const float* motion,
                                        const float* gt, const float* mask, int n, int K, int nz, int D, float scale, float* kld, float* div,
                                        float* rec, int* best, float* es_ade, float* es_fde, void* stream) {
    if (so_check("sttode_sampler_objective", mu, logvar, motion, gt, kld && div && rec && best && es_ade && es_fde, n, K, nz, D, scale)) return 1;
    hipLaunchKernelGGL(sampler_objective_kernel, dim3(n), dim3(64), so_lds_bytes(K, D), (hipStream_t)stream, mu, logvar, pmu, plogvar, motion, gt, mask, n, K,
                       nz, D, scale, kld, div, rec, best, es_ade, es_fde);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_sampler_objective_bwd(const float* mu, const float* logvar, const float* pmu, const float* plogvar,
                                            const float* motion, const float* gt, const float* mask, const float* g_kld, const float* g_div,
                                            const float* g_rec, const float* g_es_ade, const float* g_es_fde, int n, int K, int nz, int D,
                                            float scale, float* dmu, float* dlogvar, float* dmotion, void* stream) {
    if (so_check("sttode_sampler_objective_bwd", mu, logvar, motion, gt, dmu && dlogvar && dmotion, n, K, nz, D, scale)) return 1;
    hipLaunchKernelGGL(sampler_objective_bwd_kernel, dim3(n), dim3(64), so_lds_bytes(K, D), (hipStream_t)stream, mu, logvar, pmu, plogvar, motion, gt, mask,
                       g_kld, g_div, g_rec, g_es_ade, g_es_fde, n, K, nz, D, scale, dmu, dlogvar, dmotion);
    STT_HIP(hipGetLastError());
    return 0;
}
