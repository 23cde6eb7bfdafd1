// The optimizer step (train.py:122 torch.optim.Adam(model.parameters(), lr); its step at train.py:64-66,85-87) for ALL parameters of the
// model, and what goes in front of it when the caller asks: the global gradient norm, torch's clip coefficient and a non-finite guard
// (the reference carries a detect_grad_nan, core/utils.py:268-272, and never calls it), all on the device with no host round trip.
//   adam_step_kernel          the update of every parameter and both moments in ONE launch (sttode_adam_step: the default path)
//   grad_sumsq_kernel         per 1024-element chunk: sum g^2 -> partials[chunk]                          }  sttode_grad_norm
//   grad_norm_finish_kernel   one workgroup: the partials in double -> the optimizer's device state block  }
//   adam_step_guarded_kernel  adam_step_kernel on g * coef, with `apply` and the bias-correction scalars read from the state block
//   grad_scale_kernel         g *= coef in place (the stand-alone clip_grad_norm_)
// All four chunked kernels share one grid and one tensor table: block b = one 1024-element chunk of one tensor.
#include "api_util.hpp"
#include "chain.hpp"
#include "../../include/sttode_hip.h"

// ---------------------------------------------------------------------------------------------------
// Adam for ALL parameters of the model in ONE launch:
//     m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)      (g += wd p first)
// torch's fused implementation walks the 88 small tensors with multi_tensor_apply: 3 launches of 41-44 us each per step (131 us of a 2.3-ms
// NBA-size step, 140 us of a 1.05-ms one-scene step: profiles/r05/prof_train_nba_kernel_stats_before_adam.csv); the whole update moves
// 1.6 M parameters x 4 tensors = 26 MB.  Here a device table lists the tensors (parameter, first / second moment, gradient offset, element
// count, first chunk); block b finds its tensor by binary search over the chunk prefix and updates one 1024-element chunk in 16-byte pieces.
// Gradients are addressed as gbase + offset: the training engine hands out every step's gradients as views of ONE flat buffer with a fixed
// layout, so the table is uploaded once and only gbase changes.
// ---------------------------------------------------------------------------------------------------
struct AdamItem { float* p; float* m; float* v; long goff; long numel; long chunk0; };   // goff: floats from gbase; chunk0: first 1024-element chunk
#define ADAM_CHUNK 1024

// the tensor of block b: largest t with chunk0[t] <= b
static __device__ __forceinline__ AdamItem adam_item_of(const AdamItem* __restrict__ items, int n, long b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].chunk0 <= b) lo = mid; else hi = mid - 1;
    }
    return items[lo];
}

// One thread's (up to) four elements of a chunk, starting at element e0 < numel of `it`: the whole update, shared by the plain and the
// guarded kernel so that the two cannot drift apart.  coef: the clip coefficient (CLIP false: not read, g is used as it is).
template <bool CLIP>
static __device__ __forceinline__ void adam_update4(const AdamItem& it, const float* __restrict__ g, long e0, float coef, float lr_over_bc1, float omb1,
                                                    float b2, float omb2, float eps, float inv_bc2_sqrt, float wd) {
    float pv[4], mv[4], vv[4], gv[4];
    const bool vec = e0 + 3 < it.numel && ((((size_t)(it.p + e0)) | ((size_t)(it.m + e0)) | ((size_t)(it.v + e0)) | ((size_t)(g + e0))) & 15) == 0;
    const int cnt = it.numel - e0 < 4 ? (int)(it.numel - e0) : 4;
    if (vec) {
        const f32x4 P = ld4(it.p + e0), M = ld4(it.m + e0), V = ld4(it.v + e0), G = ld4(g + e0);
#pragma unroll
        for (int r = 0; r < 4; ++r) { pv[r] = P[r]; mv[r] = M[r]; vv[r] = V[r]; gv[r] = G[r]; }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r < cnt) { pv[r] = it.p[e0 + r]; mv[r] = it.m[e0 + r]; vv[r] = it.v[e0 + r]; gv[r] = g[e0 + r]; }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r >= cnt) break;
        float gr = gv[r];
        if (CLIP) gr = __fmul_rn(gr, coef);                          // (its own rounding, never contracted into what follows: coef == 1 is the plain kernel bit for bit)
        if (wd != 0.f) gr = fmaf(wd, pv[r], gr);
        mv[r] = mv[r] + omb1 * (gr - mv[r]);                         // exp_avg.lerp_(grad, 1 - beta1): 1 - beta formed in double on the host, as torch does
        vv[r] = vv[r] * b2 + omb2 * gr * gr;                         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
        const float denom = sqrtf(vv[r]) * inv_bc2_sqrt + eps;
        pv[r] = pv[r] - lr_over_bc1 * (mv[r] / denom);
    }
    if (vec) {
        st4(it.p + e0, f32x4{pv[0], pv[1], pv[2], pv[3]});
        st4(it.m + e0, f32x4{mv[0], mv[1], mv[2], mv[3]});
        st4(it.v + e0, f32x4{vv[0], vv[1], vv[2], vv[3]});
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r < cnt) { it.p[e0 + r] = pv[r]; it.m[e0 + r] = mv[r]; it.v[e0 + r] = vv[r]; }
    }
}

__global__ __launch_bounds__(256) void adam_step_kernel(const AdamItem* __restrict__ items, int n, const float* __restrict__ gbase, float lr_over_bc1,
                                                        float omb1, float b2, float omb2, float eps, float inv_bc2_sqrt, float wd) {
    const long b = blockIdx.x;
    const AdamItem it = adam_item_of(items, n, b);
    const long e0 = (b - it.chunk0) * ADAM_CHUNK + 4 * (long)threadIdx.x;
    if (e0 >= it.numel) return;
    adam_update4<false>(it, gbase + it.goff, e0, 1.f, lr_over_bc1, omb1, b2, omb2, eps, inv_bc2_sqrt, wd);
}
// items: DEVICE array of n AdamItem (6 x 8 bytes each: p, m, v pointers, goff, numel, chunk0), chunk0 ascending from 0; chunks = their total
extern "C" int sttode_adam_step(const void* items, int n, long chunks, const float* gbase, double lr, double beta1, double beta2, double eps,
                                double weight_decay, long step, void* stream) {
    STT_REQUIRE(items && n > 0 && chunks > 0 && chunks < (1L << 31) && step >= 1, "sttode_adam_step: bad argument");
    STT_REQUIRE(lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0., "sttode_adam_step: bad hyper-parameter");
    // (hyper-parameters as doubles: torch forms 1 - beta, the bias corrections and the step size in Python floats and rounds once)
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, (const AdamItem*)items, n, gbase,
                       (float)(lr / bc1), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)(1.0 / sqrt(bc2)), (float)weight_decay);
    STT_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Global-norm clipping and the non-finite guard.  The device state block (STTODE_GRAD_STATE_WORDS 32-bit words, owned by the caller, zeroed
// once) is written by ONE workgroup per step -- one writer for the counters -- and read by the update that follows it on the stream:
//   [0] total_norm (float)   [1] coef = min(1, max_norm / (total_norm + 1e-6)) (float; 1 with clipping off)   [2] apply (int)
//   [3] applied (int)   [4] skipped (int)   [8 + 2 g], [9 + 2 g]: lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t) of param group g (float)
// A step whose norm is not finite (guard on) leaves apply = 0 and counts in `skipped`; its t does not advance (t = calls - skipped), as a
// step that a GradScaler skipped.
// ---------------------------------------------------------------------------------------------------
enum { GS_NORM = 0, GS_COEF = 1, GS_APPLY = 2, GS_APPLIED = 3, GS_SKIPPED = 4, GS_SCAL = 8 };
static_assert(GS_SCAL + 2 * STTODE_GRAD_MAX_GROUPS <= STTODE_GRAD_STATE_WORDS, "state block too small");

// Sum of squares of one chunk, in a fixed order (per thread, cross-lane tree, the four waves through LDS): repeatable bit for bit, and a
// NaN / Inf in any element reaches the partial (plain sums and products only).
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const AdamItem* __restrict__ items, int n, const float* __restrict__ gbase,
                                                         float* __restrict__ partials) {
    __shared__ float wsum[4];
    const long b = blockIdx.x;
    const AdamItem it = adam_item_of(items, n, b);
    const long e0 = (b - it.chunk0) * ADAM_CHUNK + 4 * (long)threadIdx.x;
    const float* g = gbase + it.goff;
    float s = 0.f;
    if (e0 < it.numel) {                                             // (past numel: nothing is loaded; the thread still takes part in the sum)
        if (e0 + 3 < it.numel && (((size_t)(g + e0)) & 15) == 0) {
            const f32x4 G = ld4(g + e0);
            s = ((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]) + G[3] * G[3];
        } else {
            const int cnt = it.numel - e0 < 4 ? (int)(it.numel - e0) : 4;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r < cnt) s += g[e0 + r] * g[e0 + r];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[b] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

struct GradFinishArgs {                                              // per param group, by value (ngroups <= STTODE_GRAD_MAX_GROUPS)
    double lr[STTODE_GRAD_MAX_GROUPS], beta1[STTODE_GRAD_MAX_GROUPS], beta2[STTODE_GRAD_MAX_GROUPS];
    long calls[STTODE_GRAD_MAX_GROUPS];                              // the group's step count had no step been skipped (0: no Adam scalars wanted)
    float lr_over_bc1[STTODE_GRAD_MAX_GROUPS], inv_bc2_sqrt[STTODE_GRAD_MAX_GROUPS];   // ... and the host's scalars for that count
};
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const float* __restrict__ partials, long count, double max_norm, int guard,
                                                               GradFinishArgs a, int ngroups, float* __restrict__ state) {
    __shared__ double red[256];
    double s = 0.;
    for (long i = threadIdx.x; i < count; i += 256) s += (double)partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double total = sqrt(red[0]);
    const float total_f = (float)total;
    const bool finite = (__float_as_uint(total_f) & 0x7f800000u) != 0x7f800000u;   // false for NaN and +-Inf (also a norm that overflows float)
    double c = 1.;
    if (max_norm > 0.) {
        c = max_norm / (total + 1e-6);
        c = c > 1. ? 1. : c;                                         // (a NaN norm stays a NaN coefficient, as torch.clamp(max = 1) leaves it)
    }
    int* si = reinterpret_cast<int*>(state);
    const int apply = (guard && !finite) ? 0 : 1;
    const int skipped = si[GS_SKIPPED] + (apply ? 0 : 1);
    state[GS_NORM] = total_f;
    state[GS_COEF] = (float)c;
    si[GS_APPLY] = apply;
    si[GS_APPLIED] += apply;
    si[GS_SKIPPED] = skipped;
    for (int g = 0; g < ngroups; ++g) {
        if (a.calls[g] <= 0) continue;
        float s1 = a.lr_over_bc1[g], s2 = a.inv_bc2_sqrt[g];         // no step skipped so far: the host's values, the plain path's bit for bit
        if (skipped > 0) {
            const long t = a.calls[g] - skipped > 1 ? a.calls[g] - skipped : 1;
            s1 = (float)(a.lr[g] / (1.0 - pow(a.beta1[g], (double)t)));
            s2 = (float)(1.0 / sqrt(1.0 - pow(a.beta2[g], (double)t)));
        }
        state[GS_SCAL + 2 * g] = s1;
        state[GS_SCAL + 2 * g + 1] = s2;
    }
}

__global__ __launch_bounds__(256) void adam_step_guarded_kernel(const AdamItem* __restrict__ items, int n, const float* __restrict__ gbase,
                                                                const float* __restrict__ state, int group, float omb1, float b2, float omb2,
                                                                float eps, float wd) {
    if (reinterpret_cast<const int*>(state)[GS_APPLY] == 0) return; // a skipped step stores nothing
    const long b = blockIdx.x;
    const AdamItem it = adam_item_of(items, n, b);
    const long e0 = (b - it.chunk0) * ADAM_CHUNK + 4 * (long)threadIdx.x;
    if (e0 >= it.numel) return;
    adam_update4<true>(it, gbase + it.goff, e0, state[GS_COEF], state[GS_SCAL + 2 * group], omb1, b2, omb2, eps, state[GS_SCAL + 2 * group + 1], wd);
}

__global__ __launch_bounds__(256) void grad_scale_kernel(const AdamItem* __restrict__ items, int n, float* __restrict__ gbase,
                                                         const float* __restrict__ state) {
    const float coef = state[GS_COEF];
    if (coef == 1.f) return;                                         // nothing to clip: the gradients stay as they are, bit for bit
    const long b = blockIdx.x;
    const AdamItem it = adam_item_of(items, n, b);
    const long e0 = (b - it.chunk0) * ADAM_CHUNK + 4 * (long)threadIdx.x;
    if (e0 >= it.numel) return;
    float* g = gbase + it.goff;
    if (e0 + 3 < it.numel && (((size_t)(g + e0)) & 15) == 0) {
        const f32x4 G = ld4(g + e0);
        st4(g + e0, f32x4{G[0] * coef, G[1] * coef, G[2] * coef, G[3] * coef});
    } else {
        const int cnt = it.numel - e0 < 4 ? (int)(it.numel - e0) : 4;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r < cnt) g[e0 + r] *= coef;
    }
}

static int grad_group_check(const char* who, const SttodeGradGroup& g, char* msg, size_t len) {
    if (!g.items || g.n <= 0 || g.chunks <= 0 || g.chunks >= (1L << 31) || !g.gbase || g.step < 0) {
        snprintf(msg, len, "%s: bad argument in a group (null pointer, n, chunks or step)", who);
        return 1;
    }
    if (g.step > 0 && !(g.lr >= 0. && g.beta1 >= 0. && g.beta1 < 1. && g.beta2 >= 0. && g.beta2 < 1.)) {
        snprintf(msg, len, "%s: bad hyper-parameter in a group", who);
        return 1;
    }
    return 0;
}

extern "C" int sttode_grad_norm(const SttodeGradGroup* groups, int ngroups, float* partials, long partials_len, double max_norm,
                                int skip_nonfinite, void* state, void* stream) {
    STT_REQUIRE(groups && partials && state && ngroups > 0 && ngroups <= STTODE_GRAD_MAX_GROUPS, "sttode_grad_norm: bad argument");
    STT_REQUIRE(max_norm >= 0. && max_norm <= 1.7976931348623157e308, "sttode_grad_norm: max_norm must be > 0 and finite, or 0 for no clipping");
    GradFinishArgs a = {};
    long total = 0;
    char msg[160];
    for (int g = 0; g < ngroups; ++g) {
        if (grad_group_check("sttode_grad_norm", groups[g], msg, sizeof(msg))) {
            stt_set_error(msg);
            return 1;
        }
        total += groups[g].chunks;
        a.lr[g] = groups[g].lr, a.beta1[g] = groups[g].beta1, a.beta2[g] = groups[g].beta2, a.calls[g] = groups[g].step;
        if (groups[g].step > 0) {                                    // exactly sttode_adam_step's two scalars for t = step
            const double bc1 = 1.0 - pow(groups[g].beta1, (double)groups[g].step), bc2 = 1.0 - pow(groups[g].beta2, (double)groups[g].step);
            a.lr_over_bc1[g] = (float)(groups[g].lr / bc1), a.inv_bc2_sqrt[g] = (float)(1.0 / sqrt(bc2));
        }
    }
    STT_REQUIRE(total <= partials_len && total < (1L << 31), "sttode_grad_norm: partials shorter than the groups' chunks");
    long at = 0;
    for (int g = 0; g < ngroups; ++g) {                              // one launch per group's table, consecutive ranges of ONE array
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)groups[g].chunks), dim3(256), 0, (hipStream_t)stream, (const AdamItem*)groups[g].items,
                           groups[g].n, groups[g].gbase, partials + at);
        at += groups[g].chunks;
    }
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partials, total, max_norm,
                       skip_nonfinite ? 1 : 0, a, ngroups, (float*)state);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_adam_step_guarded(const void* items, int n, long chunks, const float* gbase, double beta1, double beta2, double eps,
                                        double weight_decay, const void* state, int group, void* stream) {
    STT_REQUIRE(items && gbase && state && n > 0 && chunks > 0 && chunks < (1L << 31) && group >= 0 && group < STTODE_GRAD_MAX_GROUPS,
                "sttode_adam_step_guarded: bad argument");
    STT_REQUIRE(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0., "sttode_adam_step_guarded: bad hyper-parameter");
    hipLaunchKernelGGL(adam_step_guarded_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, (const AdamItem*)items, n, gbase,
                       (const float*)state, group, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_grad_scale(const void* items, int n, long chunks, float* gbase, const void* state, void* stream) {
    STT_REQUIRE(items && gbase && state && n > 0 && chunks > 0 && chunks < (1L << 31), "sttode_grad_scale: bad argument");
    hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, (const AdamItem*)items, n, gbase,
                       (const float*)state);
    STT_HIP(hipGetLastError());
    return 0;
}
