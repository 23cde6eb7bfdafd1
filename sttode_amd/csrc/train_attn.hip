// Training step, the attention backwards (family index: train.hip): geodesic self-attention (one workgroup per (slot, head), and its
// pair-split form) and the row / column form of the op-level transformer blocks.
#include "api_util.hpp"
#include "chain.hpp"

// ---------------------------------------------------------------------------------------------------
// geodesic self-attention backward (hyptransformerlib.py:191-300 with the untransposed-scores quirk :261-265):
//   out_i = sum_j P_ij v_j,  P_ij = softmax_j( -acos(clamp(khat_i . qhat_j)) ),  rows i = keys, columns j = queries.
// one WG per (slot, head); token (l, slot) is row l*Nb + slot of qkv [L*Nb, 192] = (q | k | v); L <= 1024.
// ---------------------------------------------------------------------------------------------------
// HD = hidden_dim / 8 (4 / 8 / 16); token rows are [q | k | v] of 3 * 8 * HD floats.  HD = 8: the sums of rounds 1-4.
template <int HD>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const float* qkv, const float* dO, float* dqkv, int L, int Nb) {
    constexpr int DM = 8 * HD;
    extern __shared__ float sm[];
    float* kh = sm;              // [L][HD] normalised keys
    float* qh = kh + L * HD;      // normalised queries
    float* vv = qh + L * HD;
    float* dd = vv + L * HD;      // dO
    float* rinv = dd + L * HD;    // [L] 1 / row sum of exp
    float* rdot = rinv + L;      // [L] sum_j P_ij dP_ij
    float* kn = rdot + L;        // [L] 1/|k|
    float* qn = kn + L;          // [L] 1/|q|
    const int slot = blockIdx.x / 8, h = blockIdx.x % 8;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        const float* row = qkv + ((long)l * Nb + slot) * (3 * DM) + h * HD;
        float q[HD], k[HD], sq = 0.f, sk = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) { q[d] = row[d]; k[d] = row[DM + d]; sq += q[d] * q[d]; sk += k[d] * k[d]; }
        const float iq = 1.0f / sqrtf(sq), ik = 1.0f / sqrtf(sk);
#pragma unroll
        for (int d = 0; d < HD; ++d) {
            qh[l * HD + d] = q[d] * iq;
            kh[l * HD + d] = k[d] * ik;
            vv[l * HD + d] = row[2 * DM + d];
            dd[l * HD + d] = dO[((long)l * Nb + slot) * DM + h * HD + d];
        }
        qn[l] = iq;
        kn[l] = ik;
    }
    __syncthreads();
    const float lo = -1.0f + 1e-4f, hi = 1.0f - 1e-4f;
    // pass 1 (thread = key row i): softmax denominator, sum_j P dP, and dkhat_i
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
        float se = 0.f, sp = 0.f;
        for (int j = 0; j < L; ++j) {
            float dot = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { dot += kh[i * HD + d] * qh[j * HD + d]; dp += dd[i * HD + d] * vv[j * HD + d]; }
            const float ex = expf(-acosf(fminf(fmaxf(dot, lo), hi)));
            se += ex;
            sp += ex * dp;
        }
        rinv[i] = 1.0f / se;
        rdot[i] = sp / se;
        float dk[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) dk[d] = 0.f;
        for (int j = 0; j < L; ++j) {
            float dot = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { dot += kh[i * HD + d] * qh[j * HD + d]; dp += dd[i * HD + d] * vv[j * HD + d]; }
            const bool inside = dot > lo && dot < hi;
            const float cl = fminf(fmaxf(dot, lo), hi);
            const float P = expf(-acosf(cl)) * rinv[i];
            const float dS = P * (dp - rdot[i]);
            const float g = inside ? dS / sqrtf(1.0f - cl * cl) : 0.f;   // d(-acos x)/dx = 1/sqrt(1-x^2)
#pragma unroll
            for (int d = 0; d < HD; ++d) dk[d] += g * qh[j * HD + d];
        }
        float pr = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) pr += dk[d] * kh[i * HD + d];
        float* o = dqkv + ((long)i * Nb + slot) * (3 * DM) + DM + h * HD;
#pragma unroll
        for (int d = 0; d < HD; ++d) o[d] = (dk[d] - kh[i * HD + d] * pr) * kn[i];
    }
    __syncthreads();
    // pass 2 (thread = query column j): dqhat_j, dv_j
    for (int j = threadIdx.x; j < L; j += blockDim.x) {
        float dq[HD], dv[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) dq[d] = dv[d] = 0.f;
        for (int i = 0; i < L; ++i) {
            float dot = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { dot += kh[i * HD + d] * qh[j * HD + d]; dp += dd[i * HD + d] * vv[j * HD + d]; }
            const bool inside = dot > lo && dot < hi;
            const float cl = fminf(fmaxf(dot, lo), hi);
            const float P = expf(-acosf(cl)) * rinv[i];
            const float dS = P * (dp - rdot[i]);
            const float g = inside ? dS / sqrtf(1.0f - cl * cl) : 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { dq[d] += g * kh[i * HD + d]; dv[d] += P * dd[i * HD + d]; }
        }
        float pr = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) pr += dq[d] * qh[j * HD + d];
        float* o = dqkv + ((long)j * Nb + slot) * (3 * DM) + h * HD;
#pragma unroll
        for (int d = 0; d < HD; ++d) {
            o[d] = (dq[d] - qh[j * HD + d] * pr) * qn[j];
            o[2 * DM + d] = dv[d];
        }
    }
}
// The same backward with the L x L pair work spread over the whole workgroup (round 5): the kernel above gives every key row / query
// column ONE thread that walks all L partners three times (exp, acos, sqrt per pair) -- at the NBA training batch (L = 32: 32 active
// lanes per workgroup) 36 us per trunk, 5 % of the step.  Here a thread owns pairs (phases A, C) or one (row, d) output element (phase D);
// the per-pair terms are computed once and kept in LDS.  Every sum over partners runs in the order of the kernel above and every term
// is the same expression; only the HD-term tangent projection is a lane butterfly instead of a loop (differences at fp32 rounding).
// LDS: 3 L^2 + L (4 HD + 4) floats (L <= ~100).
template <int HD>
__global__ __launch_bounds__(256) void attn_bwd_pairs_kernel(const float* qkv, const float* dO, float* dqkv, int L, int Nb) {
    constexpr int DM = 8 * HD;
    extern __shared__ float sm[];
    float* kh = sm;
    float* qh = kh + L * HD;
    float* vv = qh + L * HD;
    float* dd = vv + L * HD;
    float* rinv = dd + L * HD;
    float* rdot = rinv + L;
    float* kn = rdot + L;
    float* qn = kn + L;
    float* E = qn + L;            // [L][L] exp(-acos(.)), then P
    float* DP = E + L * L;        // [L][L] dO_i . v_j, then g
    float* G0 = DP + L * L;       // [L][L] sqrt(1 - x^2) inside the clamp, else 0
    const int slot = blockIdx.x / 8, h = blockIdx.x % 8, t = threadIdx.x;
    for (int l = t; l < L; l += 256) {
        const float* row = qkv + ((long)l * Nb + slot) * (3 * DM) + h * HD;
        float q[HD], k[HD], sq = 0.f, sk = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) { q[d] = row[d]; k[d] = row[DM + d]; sq += q[d] * q[d]; sk += k[d] * k[d]; }
        const float iq = 1.0f / sqrtf(sq), ik = 1.0f / sqrtf(sk);
#pragma unroll
        for (int d = 0; d < HD; ++d) {
            qh[l * HD + d] = q[d] * iq;
            kh[l * HD + d] = k[d] * ik;
            vv[l * HD + d] = row[2 * DM + d];
            dd[l * HD + d] = dO[((long)l * Nb + slot) * DM + h * HD + d];
        }
        qn[l] = iq;
        kn[l] = ik;
    }
    __syncthreads();
    const float lo = -1.0f + 1e-4f, hi = 1.0f - 1e-4f;
    for (int p = t; p < L * L; p += 256) {                     // A: per pair (i = key row, j = query column)
        const int i = p / L, j = p % L;
        float dot = 0.f, dp = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) { dot += kh[i * HD + d] * qh[j * HD + d]; dp += dd[i * HD + d] * vv[j * HD + d]; }
        const bool inside = dot > lo && dot < hi;
        const float cl = fminf(fmaxf(dot, lo), hi);
        E[p] = expf(-acosf(cl));
        DP[p] = dp;
        G0[p] = inside ? sqrtf(1.0f - cl * cl) : 0.f;            // (>= 0.014 inside the clamp: 0 marks 'outside')
    }
    __syncthreads();
    for (int i = t; i < L; i += 256) {                         // B: row sums, partners in order
        float se = 0.f, sp = 0.f;
        for (int j = 0; j < L; ++j) { const float ex = E[i * L + j]; se += ex; sp += ex * DP[i * L + j]; }
        rinv[i] = 1.0f / se;
        rdot[i] = sp / se;
    }
    __syncthreads();
    for (int p = t; p < L * L; p += 256) {                     // C: P and g per pair
        const int i = p / L;
        const float P = E[p] * rinv[i];
        const float dS = P * (DP[p] - rdot[i]);
        const float g0 = G0[p];
        E[p] = P;
        DP[p] = g0 != 0.f ? dS / g0 : 0.f;                     // d(-acos x)/dx = 1/sqrt(1-x^2)
    }
    __syncthreads();
    // D: one output element per thread: (row, d); the tangent projection needs the row's HD elements: they sit in HD consecutive lanes
    for (int e0 = 0; e0 < L * HD; e0 += 256) {
        const int e = e0 + t;
        const bool on = e < L * HD;
        const int r = on ? e / HD : 0, d = e % HD;
        float dk = 0.f, dq = 0.f, dv = 0.f;
        for (int j = 0; j < L; ++j) dk += DP[r * L + j] * qh[j * HD + d];
        for (int i = 0; i < L; ++i) { dq += DP[i * L + r] * kh[i * HD + d]; dv += E[i * L + r] * dd[i * HD + d]; }
        float pk = dk * kh[r * HD + d], pq = dq * qh[r * HD + d];
#pragma unroll
        for (int sh = 1; sh < HD; sh <<= 1) { pk += __shfl_xor(pk, sh, 64); pq += __shfl_xor(pq, sh, 64); }
        if (on) {
            float* o = dqkv + ((long)r * Nb + slot) * (3 * DM) + h * HD + d;
            o[0] = (dq - qh[r * HD + d] * pq) * qn[r];
            o[DM] = (dk - kh[r * HD + d] * pk) * kn[r];
            o[2 * DM] = dv;
        }
    }
}
extern "C" int sttode_mhgsa_attn_bwd(const float* qkv, const float* dO, float* dqkv, int L, int Nb, int head_dim, void* stream) {
    STT_REQUIRE(qkv && dO && dqkv && L > 0 && Nb > 0, "sttode_mhgsa_attn_bwd: bad argument");
    STT_REQUIRE(head_dim == 4 || head_dim == 8 || head_dim == 16, "sttode_mhgsa_attn_bwd: head_dim must be 4, 8 or 16 (hidden_dim 32 / 64 / 128)");
    const size_t shm = (size_t)L * (4 * head_dim + 4) * sizeof(float);
    STT_REQUIRE(shm <= 160 * 1024, "sttode_mhgsa_attn_bwd: attention length too long for the training backward (L (4 head_dim + 4) floats of LDS)");
#define ATTB_GO(HD)                                                                                                                   \
    do {                                                                                                                              \
        STT_SET_LDS_ONCE(attn_bwd_kernel<HD>, 160 * 1024);                                                                            \
        hipLaunchKernelGGL(attn_bwd_kernel<HD>, dim3(Nb * 8), dim3(L < 256 ? ((L + 63) / 64) * 64 : 256), shm, (hipStream_t)stream, qkv, dO, dqkv, L, Nb); \
    } while (0)
    const size_t shm2 = shm + (size_t)3 * L * L * sizeof(float);
#define ATTB_PAIRS(HD)                                                                                                                \
    do {                                                                                                                              \
        STT_SET_LDS_ONCE(attn_bwd_pairs_kernel<HD>, 160 * 1024);                                                                      \
        hipLaunchKernelGGL(attn_bwd_pairs_kernel<HD>, dim3(Nb * 8), dim3(256), shm2, (hipStream_t)stream, qkv, dO, dqkv, L, Nb);        \
    } while (0)
    if (L >= 4 && shm2 <= 150 * 1024) {
        if (head_dim == 8) ATTB_PAIRS(8); else if (head_dim == 4) ATTB_PAIRS(4); else ATTB_PAIRS(16);
    } else {
        if (head_dim == 8) ATTB_GO(8); else if (head_dim == 4) ATTB_GO(4); else ATTB_GO(16);
    }
#undef ATTB_PAIRS
#undef ATTB_GO
    STT_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Backward of sttode_mhgsa_attn for any rows x cols and separate R / C / V operands (encoder.hip mhgsa_attn_kernel<8>: the op-level
// drop-ins' cross-attention over a memory of another length, and equal-length attention whose rows and columns come from different
// tensors).  Per (slot, head): rho = rscale R[r], gam = cscale C[c], x = clamp(rho^ . gam^), P = softmax_c(-acos x), out[r] = sum_c P V[c];
//   dV[c] = sum_r P dO[r];  dS = P (dO[r] . V[c] - sum_c' P dP);  g = dS / sqrt(1 - x^2) where the clamp did not bind (torch.clamp's
//   inclusive bounds), else 0;  dR[r] = rscale / |rho| (drho^ - rho^ (rho^ . drho^)) with drho^ = sum_c g gam^_c (dC likewise).
// One WG per (slot, head) owns all rows and columns: no atomics, fixed summation order.  The outputs are overwritten.
// LDS: rows (2 HD + 3) + cols (2 HD + 1) floats.
// ---------------------------------------------------------------------------------------------------
#define RC_ATT_LDS_BYTES (64 * 1024)
__global__ __launch_bounds__(256) void attn_rc_bwd_kernel(const float* __restrict__ R, const float* __restrict__ C, const float* __restrict__ V,
                                                          const float* __restrict__ dO, float* __restrict__ dR, float* __restrict__ dC,
                                                          float* __restrict__ dV, int rows, int cols, long rs_seq, long rs_b, long cs_seq,
                                                          long cs_b, long vs_seq, long vs_b, long os_seq, long os_b, float rscale, float cscale) {
    constexpr int HD = 8;
    extern __shared__ float sm[];
    float* rh = sm;                 // [rows][HD] rho^
    float* dd = rh + rows * HD;     // [rows][HD] dO
    float* rinv = dd + rows * HD;   // [rows] 1 / sum_c exp
    float* rdot = rinv + rows;      // [rows] sum_c P dP
    float* rn = rdot + rows;        // [rows] rscale / |rho|
    float* ch = rn + rows;          // [cols][HD] gam^
    float* vv = ch + cols * HD;     // [cols][HD] V
    float* cn = vv + cols * HD;     // [cols] cscale / |gam|
    const int b = blockIdx.x / 8, h = blockIdx.x % 8;
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        const float* p = R + r * rs_seq + b * rs_b + HD * h;
        const float* po = dO + r * os_seq + b * os_b + HD * h;
        float x[HD], ss = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) { x[d] = p[d] * rscale; ss += x[d] * x[d]; }
        const float nrm = sqrtf(ss);
#pragma unroll
        for (int d = 0; d < HD; ++d) { rh[r * HD + d] = x[d] / nrm; dd[r * HD + d] = po[d]; }
        rn[r] = rscale / nrm;
    }
    for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        const float* p = C + c * cs_seq + b * cs_b + HD * h;
        const float* pv = V + c * vs_seq + b * vs_b + HD * h;
        float x[HD], ss = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) { x[d] = p[d] * cscale; ss += x[d] * x[d]; }
        const float nrm = sqrtf(ss);
#pragma unroll
        for (int d = 0; d < HD; ++d) { ch[c * HD + d] = x[d] / nrm; vv[c * HD + d] = pv[d]; }
        cn[c] = cscale / nrm;
    }
    __syncthreads();
    const float lo = -1.0f + 1e-4f, hi = 1.0f - 1e-4f;
    // pass 1 (thread = row r): softmax denominator, sum_c P dP, dR[r]
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        float se = 0.f, sp = 0.f;
        for (int c = 0; c < cols; ++c) {
            float dot = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { dot += rh[r * HD + d] * ch[c * HD + d]; dp += dd[r * HD + d] * vv[c * HD + d]; }
            const float ex = expf(-acosf(fminf(fmaxf(dot, lo), hi)));
            se += ex;
            sp += ex * dp;
        }
        const float ri = 1.0f / se, rd = sp / se;
        rinv[r] = ri;
        rdot[r] = rd;
        float g[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) g[d] = 0.f;
        for (int c = 0; c < cols; ++c) {
            float dot = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { dot += rh[r * HD + d] * ch[c * HD + d]; dp += dd[r * HD + d] * vv[c * HD + d]; }
            const bool inside = dot >= lo && dot <= hi;
            const float cl = fminf(fmaxf(dot, lo), hi);
            const float P = expf(-acosf(cl)) * ri;
            const float gs = inside ? P * (dp - rd) / sqrtf(1.0f - cl * cl) : 0.f;   // d(-acos x)/dx = 1/sqrt(1-x^2)
#pragma unroll
            for (int d = 0; d < HD; ++d) g[d] += gs * ch[c * HD + d];
        }
        float pr = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) pr += g[d] * rh[r * HD + d];
        float* o = dR + r * rs_seq + b * rs_b + HD * h;
#pragma unroll
        for (int d = 0; d < HD; ++d) o[d] = (g[d] - rh[r * HD + d] * pr) * rn[r];
    }
    __syncthreads();
    // pass 2 (thread = column c): dC[c], dV[c]
    for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        float g[HD], dv[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) g[d] = dv[d] = 0.f;
        for (int r = 0; r < rows; ++r) {
            float dot = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { dot += rh[r * HD + d] * ch[c * HD + d]; dp += dd[r * HD + d] * vv[c * HD + d]; }
            const bool inside = dot >= lo && dot <= hi;
            const float cl = fminf(fmaxf(dot, lo), hi);
            const float P = expf(-acosf(cl)) * rinv[r];
            const float gs = inside ? P * (dp - rdot[r]) / sqrtf(1.0f - cl * cl) : 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { g[d] += gs * rh[r * HD + d]; dv[d] += P * dd[r * HD + d]; }
        }
        float pr = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) pr += g[d] * ch[c * HD + d];
        float* o = dC + c * cs_seq + b * cs_b + HD * h;
        float* ov = dV + c * vs_seq + b * vs_b + HD * h;
#pragma unroll
        for (int d = 0; d < HD; ++d) { o[d] = (g[d] - ch[c * HD + d] * pr) * cn[c]; ov[d] = dv[d]; }
    }
}
extern "C" int sttode_mhgsa_attn_rc_bwd(const float* R, const float* C, const float* V, const float* dO, float* dR, float* dC, float* dV,
                                        int rows, int cols, int Nb, long rs_seq, long rs_b, long cs_seq, long cs_b, long vs_seq, long vs_b,
                                        long os_seq, long os_b, float rscale, float cscale, void* stream) {
    STT_REQUIRE(R && C && V && dO && dR && dC && dV, "sttode_mhgsa_attn_rc_bwd: null pointer");
    STT_REQUIRE(rows > 0 && cols > 0 && Nb > 0 && (long)Nb * 8 <= 0x7fffffffL, "sttode_mhgsa_attn_rc_bwd: bad rows/cols/Nb");
    const size_t shm = ((size_t)rows * (2 * 8 + 3) + (size_t)cols * (2 * 8 + 1)) * sizeof(float);
    STT_REQUIRE(shm <= RC_ATT_LDS_BYTES, "sttode_mhgsa_attn_rc_bwd: rows x cols too large for the attention backward (rows (2 head_dim + 3) + "
                                         "cols (2 head_dim + 1) floats of LDS must fit 64 KiB)");
    const int mx = rows > cols ? rows : cols;
    hipLaunchKernelGGL(attn_rc_bwd_kernel, dim3(Nb * 8), dim3(mx < 256 ? ((mx + 63) / 64) * 64 : 256), shm, (hipStream_t)stream, R, C, V, dO,
                       dR, dC, dV, rows, cols, rs_seq, rs_b, cs_seq, cs_b, vs_seq, vs_b, os_seq, os_b, rscale, cscale);
    STT_HIP(hipGetLastError());
    return 0;
}
