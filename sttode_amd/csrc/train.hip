// Training-step kernels: forward-with-tape and backward of STTODENet.forward()
// (model/STTODE.py:553-568) at the reference's training shapes (one scene, n <= 32 agents, K in {1, 20};
// NBA: 32 x 11 agents) -- a few hundred to a few thousand columns, so these are GENERIC kernels, not the
// LDS-resident fused chains of the inference path.  One translation unit per kernel family:
//   train_gemm.hip    tlinear_* (generic MFMA linear layers), tgemm_* (LDS-tiled GEMM: kernel, bwd, multi, reduce), twgrad_* / tbwd
//                     (weight gradients), tsmall_multi (scene-size multi launch); the group-mode queues of all of them and
//                     sttode_tgemm_group / sttode_twgrad_defer / sttode_twgrad_flush
//   train_ewise.hip   decoder_inputs, rows_copy / rows_reduce, the element-wise op codes (ewise, with their queue), add_ln_fwd / ln_bwd,
//                     live_rows_gather
//   train_gru.hip     GRU cell forward / backward, gru_seq_* (both sizes), conv_fwd / conv_bwd
//   train_attn.hip    attn_bwd, attn_bwd_pairs (geodesic self-attention backward), attn_rc_bwd (row / column form)
//   train_trunk.hip   one encoder trunk's forward with its tape in one launch;  train_ode.hip  the ODE encoder integrators
//   train_optim.hip   adam_step, and in front of it on request: the global gradient norm, the clip coefficient, the non-finite guard
//   train.hip         (this file) the loss kernels and the fused objective, publish_values / wait_value
// Group mode (a step's independent launches queued between sttode_tgemm_group(1) and (0)): each queue lives beside the kernel it
// launches, behind one internal function declared in train_group.hpp.
#include "api_util.hpp"
#include <chrono>
#include "chain.hpp"

// ---------------------------------------------------------------------------------------------------
// losses (model/STTODE.py:372-395) -- values and their gradients; out[] slots written by single-WG reductions
// ---------------------------------------------------------------------------------------------------
static __device__ float block_sum(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}
// out[0] = scale * sum (pred - target)^2 ; dpred = 2 * scale * gscale * (pred - target)
__global__ __launch_bounds__(256) void sqerr_kernel(const float* pred, const float* target, long count, float scale, float* out, float* dpred) {
    __shared__ float red[256];
    float acc = 0.f;
    for (long i = threadIdx.x; i < count; i += 256) {
        const float d = pred[i] - target[i];
        acc += d * d;
        if (dpred) dpred[i] = 2.0f * scale * d;
    }
    const float s = block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = s * scale;
}
// KL(q || N(0, I)) in the two-distribution form (utils/dist.py:26-29 with p.sigma = 1), sum / denom, clamp_min(min_clip).
// dparams [rows, 2*zd] = gradient of the CLAMPED value (zero when the clamp is active).
// one WG per scene (scene_ptr NULL: one WG over all rows with the given denominator).  vals[s] = clamp_min(KL_s / denom_s, min_clip),
// denom_s = agents of the scene (B = 1 per scene, model/STTODE.py:378-382); dparams carries the gradient of the clamped value.
__global__ __launch_bounds__(256) void kl_kernel(const float* params, const int* scene_ptr, int rows, int zd, float denom, float min_clip,
                                                 float* vals, float* dparams) {
    __shared__ float red[256];
    const float ps = 1.0f + 1e-8f;
    const long r0 = scene_ptr ? scene_ptr[blockIdx.x] : 0, r1 = scene_ptr ? scene_ptr[blockIdx.x + 1] : rows;
    if (scene_ptr) denom = (float)(r1 - r0);
    float acc = 0.f;
    for (long i = r0 * zd + threadIdx.x; i < r1 * zd; i += 256) {
        const long r = i / zd;
        const int d = (int)(i % zd);
        const float mu = params[r * 2 * zd + d], lv = params[r * 2 * zd + zd + d];
        const float t1 = mu / ps, t2 = expf(0.5f * lv) / ps;
        acc += 0.5f * (t1 * t1 + t2 * t2) - 0.5f - logf(t2);
    }
    const float s = block_sum(acc, red) / denom;
    const bool live = s >= min_clip;   // clamp_min_: gradient passes where input >= min (torch convention)
    if (threadIdx.x == 0) vals[blockIdx.x] = live ? s : min_clip;
    if (dparams) {
        for (long i = r0 * zd + threadIdx.x; i < r1 * zd; i += 256) {
            const long r = i / zd;
            const int d = (int)(i % zd);
            const float mu = params[r * 2 * zd + d], lv = params[r * 2 * zd + zd + d];
            const float t2 = expf(0.5f * lv) / ps;
            dparams[r * 2 * zd + d] = live ? (mu / (ps * ps)) / denom : 0.f;
            dparams[r * 2 * zd + zd + d] = live ? (0.5f * t2 * t2 - 0.5f) / denom : 0.f;  // d/dlv [0.5 t2^2 - log t2], dt2/dlv = t2/2
        }
    }
}
// best-of-K: per agent min_k sum_{t,xy} (target - pred)^2 (first minimum, like torch.min), mean over agents.
// one wave per agent (lane = sample k, K <= 64), then a single-WG mean over the per-agent minima (fixed order).
__global__ __launch_bounds__(64) void diverse_agent_kernel(const float* pred, const float* target, const int* scene_ptr,
                                                           const int* agent_scene, int n, int K, int D, float* best, float* dpred) {
    const int a = blockIdx.x, lane = threadIdx.x;
    // weight of this agent in the objective: 1 / (agents of its scene) (mean over the scene, :390-395); one scene: 1 / n
    float wgt = 1.0f / (float)n;
    if (scene_ptr) { const int sc = agent_scene[a]; wgt = 1.0f / (float)(scene_ptr[sc + 1] - scene_ptr[sc]); }
    float s = 3.4e38f;
    if (lane < K) {
        s = 0.f;
        for (int d = 0; d < D; ++d) {
            const float t = target[(long)a * D + d] - pred[((long)a * K + lane) * D + d];
            s += t * t;
        }
    }
    float bs = s;
    int bk = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(bs, o, 64);
        const int ok = __shfl_xor(bk, o, 64);
        if (os < bs || (os == bs && ok < bk)) { bs = os; bk = ok; }
    }
    if (lane == 0) best[a] = bs * wgt;
    if (dpred)
        for (int i = lane; i < K * D; i += 64) {
            const int k = i / D, d = i % D;
            const long idx = ((long)a * K + k) * D + d;
            dpred[idx] = k == bk ? 2.0f * (pred[idx] - target[(long)a * D + d]) * wgt : 0.f;
        }
}
__global__ __launch_bounds__(256) void sum_kernel(const float* v, int n, float* out) {
    __shared__ float red[256];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += v[i];
    const float s = block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = s;
}
// The whole objective of forward() (model/STTODE.py:372-395,553-568) for ONE decoder pass over K1 = 1 + K samples per agent (sample 0
// decoded from the posterior draw, samples 1..K from the prior draws), in two launches:
//   objective_kernel   blocks [0, n): agent a -- squared errors of sample 0 (prediction and recovered past), best-of-K over samples
//                      1..K, and every gradient row of the agent (dpred [K1,D], drec [K1,Dp]: zero rows where a sample does not enter);
//                      blocks [n, n + nb): the KL blocks of kl_kernel;   partial sums -> scratch
//   objective_sum      fixed-order sums of the partials -> out[0..4] = (mse, recover, kl, diverse, their sum)
struct ObjArgs {
    const float* pred; const float* rec; const float* fut; const float* past; const float* qzp; const int* scene_ptr; const int* agent_scene;
    float* dpred; float* drec; float* dqzp; float* part;   // part: [3][n] agent partials, then [nb] KL values
    int n, K1, D, Dp, zd, nb;
    int kl_rows;   // != 0 (no scene_ptr: ONE KL value over all n rows): every agent's block sums its own row's KL terms into part[3 n + a] and writes
                   // the row's UNCLAMPED gradient; objective_sum adds them up, applies the clamp and -- where it is active -- zeroes dqzp.  (Round 4:
                   // one block walked all n zd terms twice, 43 us of a 2.3-ms NBA-size step.)
    float scale_mse, scale_rec, kl_denom, min_clip;
    // live form (best != nullptr; sttode_loss_objective_live): of an agent's K1 decoder columns only sample 0 (posterior: mse + recover terms)
    // and the best of the prior samples (the min over K of loss_diverse, model/STTODE.py:390-395) receive a gradient -- every other
    // column's is exactly zero.  The gradients are written for those two columns only, dpred2 [n][2][D] / drec2 [n][2][Dp] (row 1 of
    // drec2 = 0), and best [n] names the second one (1..K); dpred / drec are not written.
    int* best; float* dpred2; float* drec2;
};
// the pieces of objective_kernel, shared with the joint form below (inlined: one arithmetic, in one place)
// KL block b (same arithmetic as kl_kernel): a batch of scenes (one block per scene)
static __device__ __forceinline__ void obj_kl_block(const ObjArgs& o, int b, float* red) {
    const float ps = 1.0f + 1e-8f;
    const long r0 = o.scene_ptr ? o.scene_ptr[b] : 0, r1 = o.scene_ptr ? o.scene_ptr[b + 1] : o.n;
    const float denom = o.scene_ptr ? (float)(r1 - r0) : o.kl_denom;
    const int zd = o.zd;
    float acc = 0.f;
    for (long i = r0 * zd + threadIdx.x; i < r1 * zd; i += 256) {
        const long r = i / zd;
        const int d = (int)(i % zd);
        const float mu = o.qzp[r * 2 * zd + d], lv = o.qzp[r * 2 * zd + zd + d];
        const float t1 = mu / ps, t2 = expf(0.5f * lv) / ps;
        acc += 0.5f * (t1 * t1 + t2 * t2) - 0.5f - logf(t2);
    }
    const float sm = block_sum(acc, red) / denom;
    const bool live = sm >= o.min_clip;
    if (threadIdx.x == 0) o.part[3 * (long)o.n + b] = live ? sm : o.min_clip;
    for (long i = r0 * zd + threadIdx.x; i < r1 * zd; i += 256) {
        const long r = i / zd;
        const int d = (int)(i % zd);
        const float mu = o.qzp[r * 2 * zd + d], lv = o.qzp[r * 2 * zd + zd + d];
        const float t2 = expf(0.5f * lv) / ps;
        o.dqzp[r * 2 * zd + d] = live ? (mu / (ps * ps)) / denom : 0.f;
        o.dqzp[r * 2 * zd + zd + d] = live ? (0.5f * t2 * t2 - 0.5f) / denom : 0.f;
    }
}
// agent a, sample 0: squared errors (-> s0, s1 in every thread) + gradients; returns the agent's first gradient row of dpred
static __device__ __forceinline__ float* obj_sample0(const ObjArgs& o, int a, float* red, float& s0, float& s1) {
    const int t = threadIdx.x, K1 = o.K1, D = o.D, Dp = o.Dp;
    const float* pa = o.pred + (long)a * K1 * D;
    const float* ra = o.rec + (long)a * K1 * Dp;
    float e0 = 0.f, e1 = 0.f;
    const bool live = o.best != nullptr;
    float* dp0 = live ? o.dpred2 + (long)a * 2 * D : o.dpred + (long)a * K1 * D;
    float* dr0 = live ? o.drec2 + (long)a * 2 * Dp : o.drec + (long)a * K1 * Dp;
    for (int d = t; d < D; d += 256) { const float df = pa[d] - o.fut[(long)a * D + d]; e0 += df * df; dp0[d] = 2.0f * o.scale_mse * df; }
    for (int d = t; d < Dp; d += 256) { const float df = ra[d] - o.past[(long)a * Dp + d]; e1 += df * df; dr0[d] = 2.0f * o.scale_rec * df; }
    for (int i = Dp + t; i < (live ? 2 : K1) * Dp; i += 256) dr0[i] = 0.f;
    s0 = block_sum(e0, red);
    s1 = block_sum(e1, red);
    return dp0;
}
// agent a's row of the KL term (arithmetic of kl_kernel), gradient as if the clamp were inactive
static __device__ __forceinline__ void obj_kl_row(const ObjArgs& o, int a, float* red) {
    const int t = threadIdx.x;
    const float ps = 1.0f + 1e-8f;
    const int zd = o.zd;
    float acc = 0.f;
    for (int d = t; d < zd; d += 256) {
        const float mu = o.qzp[(long)a * 2 * zd + d], lv = o.qzp[(long)a * 2 * zd + zd + d];
        const float t1 = mu / ps, t2 = expf(0.5f * lv) / ps;
        acc += 0.5f * (t1 * t1 + t2 * t2) - 0.5f - logf(t2);
        o.dqzp[(long)a * 2 * zd + d] = (mu / (ps * ps)) / o.kl_denom;
        o.dqzp[(long)a * 2 * zd + zd + d] = (0.5f * t2 * t2 - 0.5f) / o.kl_denom;
    }
    const float sk_ = block_sum(acc, red);
    if (t == 0) o.part[3 * (long)o.n + a] = sk_;
}
__global__ __launch_bounds__(256) void objective_kernel(ObjArgs o) {
    __shared__ float red[256];
    if ((int)blockIdx.x >= o.n) {     // KL block: a batch of scenes (one block per scene) -- or the single-scene case when the agents' blocks
                                      // did not take the term over (o.kl_rows == 0)
        obj_kl_block(o, blockIdx.x - o.n, red);
        return;
    }
    const int a = blockIdx.x, t = threadIdx.x, K1 = o.K1, D = o.D;
    const float* pa = o.pred + (long)a * K1 * D;
    const bool live = o.best != nullptr;
    float s0, s1;
    float* dp0 = obj_sample0(o, a, red, s0, s1);
    // samples 1..K: first minimum of the summed squared error (torch.min), weight 1 / (agents of the scene)
    float wgt = 1.0f / (float)o.n;
    if (o.scene_ptr) { const int sc = o.agent_scene[a]; wgt = 1.0f / (float)(o.scene_ptr[sc + 1] - o.scene_ptr[sc]); }
    __shared__ float sv[64];
    __shared__ int sk;
    if (t < 64) {
        float sq = 3.4e38f;
        if (t + 1 < K1) {
            sq = 0.f;
            for (int d = 0; d < D; ++d) { const float df = o.fut[(long)a * D + d] - pa[(long)(t + 1) * D + d]; sq += df * df; }
        }
        float bs = sq;
        int bk = t;
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) {
            const float os = __shfl_xor(bs, sh, 64);
            const int ok = __shfl_xor(bk, sh, 64);
            if (os < bs || (os == bs && ok < bk)) { bs = os; bk = ok; }
        }
        if (t == 0) { sv[0] = bs; sk = bk; }
    }
    __syncthreads();
    const int bk = sk + 1;
    if (live) {
        for (int d = t; d < D; d += 256) dp0[D + d] = 2.0f * (pa[(long)bk * D + d] - o.fut[(long)a * D + d]) * wgt;
        if (t == 0) o.best[a] = bk;
    } else {
        for (int i = D + t; i < K1 * D; i += 256) {
            const int k = i / D, d = i % D;
            o.dpred[(long)a * K1 * D + i] = k == bk ? 2.0f * (pa[i] - o.fut[(long)a * D + d]) * wgt : 0.f;
        }
    }
    if (t == 0) { o.part[a] = s0; o.part[o.n + a] = s1; o.part[2 * (long)o.n + a] = sv[0] * wgt; }
    if (o.kl_rows) obj_kl_row(o, a, red);
}
__global__ __launch_bounds__(256) void objective_sum_kernel(const float* part, int n, int nb, float scale_mse, float scale_rec, float* out,
                                                           int kl_rows, float kl_denom, float min_clip, float* dqzp, int zd) {
    __shared__ float red[256];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { a0 += part[i]; a1 += part[n + i]; a2 += part[2 * (long)n + i]; }
    for (int i = threadIdx.x; i < (kl_rows ? kl_rows : nb); i += 256) a3 += part[3 * (long)n + i];
    const float s0 = block_sum(a0, red), s1 = block_sum(a1, red), s2 = block_sum(a2, red);
    float s3 = block_sum(a3, red);
    if (kl_rows) {                    // (uniform) the agents' row sums -> clamp_min(KL / denom, min_clip); an active clamp passes no gradient
        s3 /= kl_denom;
        const bool live = s3 >= min_clip;
        if (!live) {
            s3 = min_clip;
            for (long i = threadIdx.x; i < (long)kl_rows * 2 * zd; i += 256) dqzp[i] = 0.f;
        }
    }
    if (threadIdx.x == 0) {
        const float l0 = s0 * scale_mse, l1 = s1 * scale_rec;
        out[0] = l0; out[1] = l1; out[2] = s3; out[3] = s2;
        out[4] = ((l0 + l1) + s3) + s2;   // total_loss (model/STTODE.py:568)
    }
}
static int loss_objective_impl(const float* pred, const float* rec, const float* fut, const float* past, const float* qzp,
                               const int* scene_ptr, const int* agent_scene, int S, int n, int K1, int D, int Dp, int zd,
                               float scale_mse, float scale_rec, float kl_denom, float min_clip, float* out, float* dpred,
                               float* drec, float* dqzp, int* best, float* scratch, long scratch_floats, void* stream) {
    STT_REQUIRE(pred && rec && fut && past && qzp && out && dpred && drec && dqzp && scratch, "sttode_loss_objective: null pointer");
    STT_REQUIRE(n > 0 && K1 >= 2 && K1 <= 65 && D > 0 && Dp > 0 && zd > 0, "sttode_loss_objective: bad sizes (2 <= K1 <= 65)");
    STT_REQUIRE(scene_ptr ? (S > 0 && agent_scene) : kl_denom > 0.f, "sttode_loss_objective: scene_ptr needs S > 0 and agent_scene, otherwise kl_denom > 0");
    const int nb = scene_ptr ? S : 0;             // KL blocks: one per scene of a batch; the single-value case rides in the agents' blocks
    const int kl_rows = scene_ptr ? 0 : n;
    STT_REQUIRE(3L * n + (scene_ptr ? S : n) <= scratch_floats, "sttode_loss_objective: scratch too small (3 n + max(S, n) floats)");
    ObjArgs o;
    o.pred = pred; o.rec = rec; o.fut = fut; o.past = past; o.qzp = qzp; o.scene_ptr = scene_ptr; o.agent_scene = agent_scene;
    o.dpred = best ? nullptr : dpred; o.drec = best ? nullptr : drec; o.dqzp = dqzp; o.part = scratch;
    o.best = best; o.dpred2 = best ? dpred : nullptr; o.drec2 = best ? drec : nullptr;
    o.n = n; o.K1 = K1; o.D = D; o.Dp = Dp; o.zd = zd; o.nb = nb; o.kl_rows = kl_rows;
    o.scale_mse = scale_mse; o.scale_rec = scale_rec; o.kl_denom = kl_denom; o.min_clip = min_clip;
    hipLaunchKernelGGL(objective_kernel, dim3(n + nb), dim3(256), 0, (hipStream_t)stream, o);
    hipLaunchKernelGGL(objective_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scratch, n, nb, scale_mse, scale_rec, out, kl_rows, kl_denom,
                       min_clip, dqzp, zd);
    STT_HIP(hipGetLastError());
    return 0;
}
extern "C" int sttode_loss_objective(const float* pred, const float* rec, const float* fut, const float* past, const float* qzp,
                                     const int* scene_ptr, const int* agent_scene, int S, int n, int K1, int D, int Dp, int zd,
                                     float scale_mse, float scale_rec, float kl_denom, float min_clip, float* out, float* dpred,
                                     float* drec, float* dqzp, float* scratch, long scratch_floats, void* stream) {
    return loss_objective_impl(pred, rec, fut, past, qzp, scene_ptr, agent_scene, S, n, K1, D, Dp, zd, scale_mse, scale_rec, kl_denom, min_clip, out,
                               dpred, drec, dqzp, nullptr, scratch, scratch_floats, stream);
}
extern "C" int sttode_loss_objective_live(const float* pred, const float* rec, const float* fut, const float* past, const float* qzp,
                                          const int* scene_ptr, const int* agent_scene, int S, int n, int K1, int D, int Dp, int zd,
                                          float scale_mse, float scale_rec, float kl_denom, float min_clip, float* out, float* dpred2,
                                          float* drec2, float* dqzp, int* best, float* scratch, long scratch_floats, void* stream) {
    STT_REQUIRE(best, "sttode_loss_objective_live: null pointer");
    return loss_objective_impl(pred, rec, fut, past, qzp, scene_ptr, agent_scene, S, n, K1, D, Dp, zd, scale_mse, scale_rec, kl_denom, min_clip, out,
                               dpred2, drec2, dqzp, best, scratch, scratch_floats, stream);
}

// ---------------------------------------------------------------------------------------------------
// The scene-level (joint) best-of-K term: the min over the K prior samples is taken OUTSIDE the sum over a segment's agents
// (a scene of a CSR batch, all agents of one scene, one NBA game) -- every agent of a segment selects the same sample k*_g.
//   J_g(k) = sum_{a in g} sq_a(k),   k*_g = first k minimising J_g,   term = sum_g w_g J_g(k*_g),   w_g = the marginal form's agent weight
// One workgroup per segment, no block depends on another: lane <-> sample (K <= 64 = one wave), the four waves split the segment's agents
// (wave w: agents r0 + w, r0 + w + 4, ...); sq_a(k) in fp32 in the marginal kernel's order, their sum over the wave's agents in double in
// agent order, the four wave sums added in wave order, then the marginal kernel's first-minimum butterfly on the doubles.  A segment's
// outputs depend on its own agents only -- not on the other segments, not on where it stands in the batch.
// part[r0] = the segment's weighted value, part[r0 + 1 .. r1) = 0: the fixed-order sums over n slots (objective_sum_kernel, sum_kernel)
// serve unchanged, and one-agent segments reproduce the marginal term bit for bit.
// pred: agent a's K prior columns are rows a KS + k0 .. a KS + k0 + K - 1 of D floats.  Gradients: row1 != NULL -> [n][2][D], row 1 (the live
// form); dense != NULL -> [n][K][D], zero rows but the selected one.  best / seg_best: 1..K.
// ---------------------------------------------------------------------------------------------------
static __device__ __forceinline__ void joint_segment(const float* pred, const float* fut, int KS, int k0, int K, int D, int r0, int r1,
                                                     float wgt, float* part, float* row1, float* dense, int* best, int* seg_best) {
    __shared__ double sj[4][64];
    __shared__ int sk;
    __shared__ float sval;
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    double acc = 0.0;
    if (lane < K)
        for (int a = r0 + w; a < r1; a += 8) {      // two of the wave's agents per pass, their loads in flight together (one scene: the
                                                    // segment's n agents wait on this one workgroup); each sum and the order of acc as one by one
            const int a2 = a + 4 < r1 ? a + 4 : a;
            const float* pa = pred + ((long)a * KS + k0 + lane) * D;
            const float* pb = pred + ((long)a2 * KS + k0 + lane) * D;
            const float* fa = fut + (long)a * D;
            const float* fb = fut + (long)a2 * D;
            float sq = 0.f, sq2 = 0.f;
#pragma unroll 4
            for (int d = 0; d < D; ++d) {
                const float df = fa[d] - pa[d], df2 = fb[d] - pb[d];
                sq += df * df;
                sq2 += df2 * df2;
            }
            acc += (double)sq;
            if (a2 != a) acc += (double)sq2;
        }
    sj[w][lane] = acc;
    __syncthreads();
    if (w == 0) {
        double bs = lane < K ? ((sj[0][lane] + sj[1][lane]) + sj[2][lane]) + sj[3][lane] : __builtin_huge_val();
        int bk = lane;
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) {
            const double os = __shfl_xor(bs, sh, 64);
            const int ok = __shfl_xor(bk, sh, 64);
            if (os < bs || (os == bs && ok < bk)) { bs = os; bk = ok; }
        }
        if (lane == 0) { sk = bk; sval = (float)(bs * (double)wgt); }   // (lane 0 always ends on a lane < K, whatever the values: see DESIGN.md 4v)
    }
    __syncthreads();
    const int bk = sk, cnt = r1 - r0;
    if (row1)
        for (long i = t; i < (long)cnt * D; i += 256) {
            const long a = r0 + i / D;
            const int d = (int)(i % D);
            row1[(a * 2 + 1) * D + d] = 2.0f * (pred[(a * KS + k0 + bk) * D + d] - fut[a * D + d]) * wgt;
        }
    if (dense)
        for (long i = t; i < (long)cnt * K * D; i += 256) {
            const long a = r0 + i / ((long)K * D);
            const int k = (int)(i / D % K), d = (int)(i % D);
            dense[(long)r0 * K * D + i] = k == bk ? 2.0f * (pred[(a * KS + k0 + k) * D + d] - fut[a * D + d]) * wgt : 0.f;
        }
    for (int i = t; i < cnt; i += 256) {
        if (best) best[r0 + i] = bk + 1;
        part[r0 + i] = i == 0 ? sval : 0.f;
    }
    if (seg_best && t == 0) *seg_best = bk + 1;
}
// The objective with the joint term, live form: blocks [0, n) the agents' sample-0 work (and their KL rows), [n, n + nb) the KL blocks of a
// batch of scenes -- both exactly objective_kernel's -- and [n + nb, n + nb + G) one workgroup per segment.
__global__ __launch_bounds__(256) void objective_joint_kernel(ObjArgs o, int seg_len, int* seg_best) {
    __shared__ float red[256];
    const int b = blockIdx.x;
    if (b >= o.n + o.nb) {
        const int g = b - o.n - o.nb;
        const int r0 = o.scene_ptr ? o.scene_ptr[g] : g * seg_len, r1 = o.scene_ptr ? o.scene_ptr[g + 1] : r0 + seg_len;
        const float wgt = 1.0f / (float)(o.scene_ptr ? r1 - r0 : o.n);
        joint_segment(o.pred, o.fut, o.K1, 1, o.K1 - 1, o.D, r0, r1, wgt, o.part + 2 * (long)o.n, o.dpred2, nullptr, o.best,
                      seg_best ? seg_best + g : nullptr);
        return;
    }
    if (b >= o.n) {
        obj_kl_block(o, b - o.n, red);
        return;
    }
    float s0, s1;
    obj_sample0(o, b, red, s0, s1);
    if (threadIdx.x == 0) { o.part[b] = s0; o.part[o.n + b] = s1; }
    if (o.kl_rows) obj_kl_row(o, b, red);
}
// the term alone: one workgroup per possible segment (with a CSR the host does not know S: agent_scene[n - 1] + 1)
__global__ __launch_bounds__(256) void diverse_joint_kernel(const float* pred, const float* target, const int* scene_ptr, const int* agent_scene,
                                                            int n, int K, int D, int seg_len, float* part, float* dpred, int* best) {
    const int g = blockIdx.x;
    if (g >= (scene_ptr ? agent_scene[n - 1] + 1 : n / seg_len)) return;
    const int r0 = scene_ptr ? scene_ptr[g] : g * seg_len, r1 = scene_ptr ? scene_ptr[g + 1] : r0 + seg_len;
    const float wgt = 1.0f / (float)(scene_ptr ? r1 - r0 : n);
    joint_segment(pred, target, K, 0, K, D, r0, r1, wgt, part, nullptr, dpred, best, nullptr);
}
extern "C" int sttode_loss_objective_joint(const float* pred, const float* rec, const float* fut, const float* past, const float* qzp,
                                           const int* scene_ptr, const int* agent_scene, int S, int n, int K1, int D, int Dp, int zd,
                                           float scale_mse, float scale_rec, float kl_denom, float min_clip, float* out, float* dpred2,
                                           float* drec2, float* dqzp, int* best, int seg_len, int* seg_best, float* scratch,
                                           long scratch_floats, void* stream) {
    STT_REQUIRE(pred && rec && fut && past && qzp && out && dpred2 && drec2 && dqzp && best && scratch, "sttode_loss_objective_joint: null pointer");
    STT_REQUIRE(n > 0 && K1 >= 2 && K1 <= 65 && D > 0 && Dp > 0 && zd > 0, "sttode_loss_objective_joint: bad sizes (2 <= K1 <= 65)");
    STT_REQUIRE(scene_ptr ? (S > 0 && agent_scene) : kl_denom > 0.f,
                "sttode_loss_objective_joint: scene_ptr needs S > 0 and agent_scene, otherwise kl_denom > 0");
    STT_REQUIRE(scene_ptr ? seg_len == 0 : (seg_len >= 1 && n % seg_len == 0),
                "sttode_loss_objective_joint: bad seg_len (0 with scene_ptr: the segments are the scenes; otherwise >= 1 and a divisor of n)");
    STT_REQUIRE(3L * n + (scene_ptr ? S : n) <= scratch_floats, "sttode_loss_objective_joint: scratch too small (3 n + max(S, n) floats)");
    const int nb = scene_ptr ? S : 0, kl_rows = scene_ptr ? 0 : n, G = scene_ptr ? S : n / seg_len;
    ObjArgs o;
    o.pred = pred; o.rec = rec; o.fut = fut; o.past = past; o.qzp = qzp; o.scene_ptr = scene_ptr; o.agent_scene = agent_scene;
    o.dpred = nullptr; o.drec = nullptr; o.dqzp = dqzp; o.part = scratch;
    o.best = best; o.dpred2 = dpred2; o.drec2 = drec2;
    o.n = n; o.K1 = K1; o.D = D; o.Dp = Dp; o.zd = zd; o.nb = nb; o.kl_rows = kl_rows;
    o.scale_mse = scale_mse; o.scale_rec = scale_rec; o.kl_denom = kl_denom; o.min_clip = min_clip;
    hipLaunchKernelGGL(objective_joint_kernel, dim3(n + nb + G), dim3(256), 0, (hipStream_t)stream, o, seg_len, seg_best);
    hipLaunchKernelGGL(objective_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scratch, n, nb, scale_mse, scale_rec, out, kl_rows, kl_denom,
                       min_clip, dqzp, zd);
    STT_HIP(hipGetLastError());
    return 0;
}
extern "C" int sttode_loss_diverse_joint(const float* pred, const float* target, const int* scene_ptr, const int* agent_scene, int n, int K,
                                         int D, int seg_len, float* out, float* dpred, int* best, float* scratch, void* stream) {
    STT_REQUIRE(pred && target && out && scratch && n > 0 && K > 0 && K <= 64 && D > 0,
                "sttode_loss_diverse_joint: bad argument (1 <= K <= 64, scratch >= n floats)");
    STT_REQUIRE(!scene_ptr || agent_scene, "sttode_loss_diverse_joint: scene_ptr needs agent_scene");
    STT_REQUIRE(scene_ptr ? seg_len == 0 : (seg_len >= 1 && n % seg_len == 0),
                "sttode_loss_diverse_joint: bad seg_len (0 with scene_ptr: the segments are the scenes; otherwise >= 1 and a divisor of n)");
    hipLaunchKernelGGL(diverse_joint_kernel, dim3(scene_ptr ? n : n / seg_len), dim3(256), 0, (hipStream_t)stream, pred, target, scene_ptr,
                       agent_scene, n, K, D, seg_len, scratch, dpred, best);
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scratch, n, out);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_loss_sqerr(const float* pred, const float* target, long count, float scale, float* out, float* dpred, void* stream) {
    STT_REQUIRE(pred && target && out && count > 0, "sttode_loss_sqerr: bad argument");
    hipLaunchKernelGGL(sqerr_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pred, target, count, scale, out, dpred);
    STT_HIP(hipGetLastError());
    return 0;
}
extern "C" int sttode_loss_kl(const float* params, const int* scene_ptr, int S, int rows, int zd, float denom, float min_clip, float* out,
                              float* dparams, float* scratch, void* stream) {
    STT_REQUIRE(params && out && scratch && rows > 0 && zd > 0, "sttode_loss_kl: bad argument");
    STT_REQUIRE(scene_ptr ? S > 0 : denom > 0.f, "sttode_loss_kl: scene_ptr needs S > 0, otherwise denom > 0");
    const int nb = scene_ptr ? S : 1;
    hipLaunchKernelGGL(kl_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, params, scene_ptr, rows, zd, denom, min_clip, scratch, dparams);
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scratch, nb, out);
    STT_HIP(hipGetLastError());
    return 0;
}
extern "C" int sttode_loss_diverse(const float* pred, const float* target, const int* scene_ptr, const int* agent_scene, int n, int K,
                                   int D, float* out, float* dpred, float* scratch, void* stream) {
    STT_REQUIRE(pred && target && out && scratch && n > 0 && K > 0 && K <= 64 && D > 0, "sttode_loss_diverse: bad argument (K <= 64, scratch >= n floats)");
    STT_REQUIRE(!scene_ptr || agent_scene, "sttode_loss_diverse: scene_ptr needs agent_scene");
    hipLaunchKernelGGL(diverse_agent_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, pred, target, scene_ptr, agent_scene, n, K, D, scratch, dpred);
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scratch, n, out);
    STT_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Values a replayed step hands to the HOST in the middle of its graph (STTODENet.forward() returns four Python floats,
// model/STTODE.py:568 -- `.item()` there is a device synchronisation at the END of whatever is queued; the loss values exist after the
// forward half of the step).  publish: one lane copies n values into pinned host memory with system-scope stores, then bumps a DEVICE
// counter (a replayed graph cannot carry a per-replay argument) and stores the new count into the host's sequence word (release).
// wait: the host spins on that word -- no stream or event is involved, so the rest of the graph (the backward pass) keeps running
// while the caller goes on to zero_grad / backward / optimizer.step and queues them behind it.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void publish_kernel(const float* __restrict__ vals, int n, float* host_vals, unsigned* dev_seq, unsigned* host_seq) {
    if (threadIdx.x != 0) return;
    for (int i = 0; i < n; ++i) __hip_atomic_store(host_vals + i, vals[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned s = *dev_seq + 1u;
    *dev_seq = s;
    __hip_atomic_store(host_seq, s, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
extern "C" int sttode_publish_values(const float* vals, int n, float* host_vals, unsigned* dev_seq, unsigned* host_seq, void* stream) {
    STT_REQUIRE(vals && host_vals && dev_seq && host_seq && n > 0 && n <= 64, "sttode_publish_values: null pointer or n outside 1..64");
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, vals, n, host_vals, dev_seq, host_seq);
    STT_HIP(hipGetLastError());
    return 0;
}
extern "C" int sttode_wait_value(const unsigned* host_seq, long want, double timeout_s) {
    STT_REQUIRE(host_seq && timeout_s > 0, "sttode_wait_value: null pointer or no time-out");
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        if (__atomic_load_n(host_seq, __ATOMIC_ACQUIRE) == (unsigned)want) return 0;
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
        if ((spins & 1023u) == 1023u &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) {
            stt_set_error("sttode_wait_value: the sequence word did not reach the expected count in time");
            return 1;
        }
    }
}
