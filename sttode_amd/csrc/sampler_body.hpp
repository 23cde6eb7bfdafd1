// Device pieces shared by the stage-2 sampler's loss kernels (sampler.hip, sampler_objective.hip, sampler_joint.hip): their
// kld, best sample and ground-truth sums agree to the bit because they are this text.
#pragma once
#include "set_body.hpp"

// KL(q || p) of agent a's K nz latents (utils/dist.py:26-29), float32: element i on lane i mod 64, a lane's elements in ascending order, the
// lanes by wave_sum.  pmu / plogvar may be null (a standard normal prior).  One wave.
__device__ __forceinline__ float sampler_kld(const float* __restrict__ mu, const float* __restrict__ logvar, const float* __restrict__ pmu,
                                             const float* __restrict__ plogvar, int a, int K, int nz, int lane) {
    float kl = 0.f;
    const size_t base = (size_t)a * K * nz;
    for (int i = lane; i < K * nz; i += 64) {
        const float m = mu[base + i], sg = expf(0.5f * logvar[base + i]);
        const float pm = pmu ? pmu[base + i] : 0.f;
        const float ps = (plogvar ? expf(0.5f * plogvar[base + i]) : 1.f) + 1e-8f;
        const float t1 = (m - pm) / ps, t2 = sg / ps;
        kl += 0.5f * (t1 * t1 + t2 * t2) - 0.5f - logf(t2);
    }
    return wave_sum(kl);
}

// motion of agent a -> sM [K][D], ground truth -> sY [D], mask -> sW [D / 2] (ones without a mask) by the workgroup's nt threads; a barrier.
__device__ __forceinline__ void sampler_stage(const float* __restrict__ motion, const float* __restrict__ gt, const float* __restrict__ mask,
                                              int a, int K, int D, int tid, int nt, float* sM, float* sY, float* sW) {
    for (int i = tid; i < K * D; i += nt) sM[i] = motion[(size_t)a * K * D + i];
    for (int i = tid; i < D; i += nt) sY[i] = gt[(size_t)a * D + i];
    for (int i = tid; i < D / 2; i += nt) sW[i] = mask ? mask[(size_t)a * (D / 2) + i] : 1.f;
    __syncthreads();
}

// Sample k against the ground truth, frames in frame order, float64: returns sum_t (m_t (x_k,t - y_t))^2; the displacements
// |m_t (x_k,t - y_t)| are added to ga and the last frame's is left in last.
__device__ __forceinline__ double sampler_gt_sample(const float* sM, const float* sY, const float* sW, int k, int D, double& ga, double& last) {
    double r2 = 0.0;
    for (int t = 0; t < D / 2; ++t) {
        const double m = (double)sW[t];
        const double ex = m * ((double)sM[k * D + 2 * t] - (double)sY[2 * t]);
        const double ey = m * ((double)sM[k * D + 2 * t + 1] - (double)sY[2 * t + 1]);
        const double d2 = ex * ex + ey * ey;
        r2 += d2;
        last = sqrt(d2);
        ga += last;
    }
    return r2;
}
