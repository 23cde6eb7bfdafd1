// Attention core with a running maximum: two score modes and an optional additive mask, forward and backward.
//   mode 0 (geodesic, hyptransformerlib.py:251-300)   s_ij = -acos(clamp(<r^_i, c^_j>, -1+1e-4, 1-1e-4)),  r = rscale R, c = cscale C, ^ = / |.|
//   mode 1 (dot product, transformerlib.py:251-282)   s_ij = <rscale R_i, cscale C_j>
//   masked                                            s_ij += mask[i * ld_mask + j]   (fp32 [rows, cols], +-inf allowed, shared by slots and heads)
//   out_i = sum_j softmax_j(s_ij) V_j                 8 heads x 8 dims; element (seq s, slot b, feature f) at base + s*seq_stride + b*b_stride + f
// encoder.hip's mhgsa_attn_kernel needs no maximum because its scores lie in [-pi, 0]; a mask or a dot product breaks that bound, so these
// kernels carry (m, l, acc) per lane.  A row whose scores are -inf over ALL columns ends with l == 0 and a NaN output row (torch's softmax
// does the same); a tile, or a leading run of tiles, that is -inf for a row leaves it untouched: exp(-inf - (-inf)) is never evaluated,
// because the subtracted maximum is replaced by 0 while it is still -inf.
#include "api_util.hpp"
#include "../../include/sttode_hip.h"

#define AC_TJ 128
#define AC_HD 8
#define AC_LOG2E 1.4426950408889634f
#define AC_NINF (-__builtin_inff())
typedef float ac_f4 __attribute__((ext_vector_type(4)));

// -acos(x) for x in [-1+1e-4, 1-1e-4]: the minimax form of encoder.hip's exp_neg_acos (Abramowitz & Stegun 4.4.46, |error| <= 2e-8)
__device__ __forceinline__ float ac_neg_acos(float x) {
    const float ax = fabsf(x);
    float p = -0.0012624911f;
    p = fmaf(p, ax, 0.0066700901f);
    p = fmaf(p, ax, -0.0170881256f);
    p = fmaf(p, ax, 0.0308918810f);
    p = fmaf(p, ax, -0.0501743046f);
    p = fmaf(p, ax, 0.0889789874f);
    p = fmaf(p, ax, -0.2145988016f);
    p = fmaf(p, ax, 1.5707963050f);
    const float a = __builtin_amdgcn_sqrtf(1.0f - ax) * p;
    return x < 0.f ? a - 3.14159265358979f : -a;
}
__device__ __forceinline__ float ac_exp(float x) { return __builtin_amdgcn_exp2f(x * AC_LOG2E); }   // v_exp_f32; exp(-inf) = 0
// the maximum to subtract: 0 while everything seen so far is -inf
__device__ __forceinline__ float ac_safe(float m) { return m == AC_NINF ? 0.f : m; }

// r[d] = scale * p[d], normalised in mode 0
template <int MODE>
__device__ __forceinline__ void ac_load(const float* p, float scale, float (&r)[AC_HD]) {
    float ss = 0.f;
#pragma unroll
    for (int d = 0; d < AC_HD; ++d) { r[d] = p[d] * scale; ss += r[d] * r[d]; }
    if (MODE == 0) {
        const float nrm = sqrtf(ss);
#pragma unroll
        for (int d = 0; d < AC_HD; ++d) r[d] = r[d] / nrm;
    }
}
template <int MODE>
__device__ __forceinline__ float ac_score(float dot) {
    return MODE == 0 ? ac_neg_acos(fminf(fmaxf(dot, -1.0f + 1e-4f), 1.0f - 1e-4f)) : dot;
}

// Forward.  The tiling of mhgsa_attn_kernel: a workgroup takes 64 rows (one per lane), its four waves split every 128-column tile (wave w:
// columns 32 w .. 32 w + 31), eight columns at a time: eight scores, their maximum joined with the running one, ONE rescale of (l, acc), eight
// exponentials.  The four (m, l, acc) partials of a row are merged through LDS in wave order 0, 1, 2, 3: the same bits on every run.
// The mask tile [64 rows][128 columns] is staged through LDS: the loads walk a mask row (coalesced, 512 B per row), the reads walk a
// column of the tile (one row per lane; the pitch of 129 floats keeps the 32 lanes of a half-wave on 32 different banks).  Read straight from
// global memory every lane would touch its own cache line per column.
template <int MODE, bool MASKED>
__global__ __launch_bounds__(256) void attn_core_kernel(const float* __restrict__ R, const float* __restrict__ C, const float* __restrict__ V,
                                                        const float* __restrict__ mask, long ld_mask, float* __restrict__ out,
                                                        float* __restrict__ wmax, float* __restrict__ wsum, int rows, int cols, long rs_seq,
                                                        long rs_b, long cs_seq, long cs_b, long vs_seq, long vs_b, long os_seq, long os_b,
                                                        float rscale, float cscale) {
    constexpr int HD = AC_HD;
    __shared__ __attribute__((aligned(16))) float sC[AC_TJ][HD];
    __shared__ __attribute__((aligned(16))) float sV[AC_TJ][HD];
    __shared__ float sP[3][64][HD + 3];                              // partials of waves 1..3: m, l, acc[HD] (odd pitch)
    __shared__ float sM[MASKED ? 64 : 1][AC_TJ + 1];
    const int bh = blockIdx.y, b = bh >> 3, h = bh & 7;
    const int rl = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i0 = blockIdx.x * 64, i = i0 + rl;
    const int ic = i < rows ? i : rows - 1;
    float r[HD];
    ac_load<MODE>(R + ic * rs_seq + b * rs_b + HD * h, rscale, r);
    float acc[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] = 0.f;
    float m = AC_NINF, l = 0.f;
    for (int j0 = 0; j0 < cols; j0 += AC_TJ) {
        __syncthreads();
        if (threadIdx.x < AC_TJ) {
            const int j = j0 + threadIdx.x;
            float v[HD];
            if (j < cols) {
                ac_load<MODE>(C + j * cs_seq + b * cs_b + HD * h, cscale, v);
            } else {
#pragma unroll
                for (int d = 0; d < HD; ++d) v[d] = 0.f;
            }
#pragma unroll
            for (int d = 0; d < HD; ++d) sC[threadIdx.x][d] = v[d];
        } else {
            const int jj = threadIdx.x - AC_TJ, j = j0 + jj;
            const float* p = V + (j < cols ? j : 0) * vs_seq + b * vs_b + HD * h;
#pragma unroll
            for (int d = 0; d < HD; ++d) sV[jj][d] = j < cols ? p[d] : 0.f;      // zero, not stale: 0 * p stays 0 behind the last column
        }
        if (MASKED) {
            const int c = threadIdx.x & (AC_TJ - 1);
            for (int rr = threadIdx.x >> 7; rr < 64; rr += 2)
                sM[rr][c] = (i0 + rr < rows && j0 + c < cols) ? mask[(long)(i0 + rr) * ld_mask + j0 + c] : 0.f;
        }
        __syncthreads();
        const int jn = min(AC_TJ, cols - j0);
#pragma unroll 1
        for (int jb = 32 * w; jb < 32 * w + 32 && jb < jn; jb += 8) {          // wave-uniform bounds
            float s[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int jj = jb + k;
                // all lanes of a wave read the same column (LDS broadcast)
                const ac_f4 c0 = *reinterpret_cast<const ac_f4*>(&sC[jj][0]), c1 = *reinterpret_cast<const ac_f4*>(&sC[jj][4]);
                float dot = r[0] * c0[0];
                dot = fmaf(r[1], c0[1], dot); dot = fmaf(r[2], c0[2], dot); dot = fmaf(r[3], c0[3], dot);
                dot = fmaf(r[4], c1[0], dot); dot = fmaf(r[5], c1[1], dot); dot = fmaf(r[6], c1[2], dot); dot = fmaf(r[7], c1[3], dot);
                float sc = ac_score<MODE>(dot);
                if (MASKED) sc += sM[rl][jj];
                s[k] = jj < jn ? sc : AC_NINF;
            }
            float mx = m;
#pragma unroll
            for (int k = 0; k < 8; ++k) mx = fmaxf(mx, s[k]);
            const float ms = ac_safe(mx);
            const float alpha = ac_exp(m - ms);
            l *= alpha;
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] *= alpha;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int jj = jb + k;
                const ac_f4 v0 = *reinterpret_cast<const ac_f4*>(&sV[jj][0]), v1 = *reinterpret_cast<const ac_f4*>(&sV[jj][4]);
                const float p = ac_exp(s[k] - ms);
                l += p;
                acc[0] = fmaf(p, v0[0], acc[0]); acc[1] = fmaf(p, v0[1], acc[1]); acc[2] = fmaf(p, v0[2], acc[2]); acc[3] = fmaf(p, v0[3], acc[3]);
                acc[4] = fmaf(p, v1[0], acc[4]); acc[5] = fmaf(p, v1[1], acc[5]); acc[6] = fmaf(p, v1[2], acc[6]); acc[7] = fmaf(p, v1[3], acc[7]);
            }
            m = mx;
        }
    }
    if (w > 0) {
        sP[w - 1][rl][0] = m;
        sP[w - 1][rl][1] = l;
#pragma unroll
        for (int d = 0; d < HD; ++d) sP[w - 1][rl][2 + d] = acc[d];
    }
    __syncthreads();
    if (w == 0 && i < rows) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                // wave order 0, 1, 2, 3
            const float mk = sP[k][rl][0];
            const float mx = fmaxf(m, mk), ms = ac_safe(mx);
            const float a = ac_exp(m - ms), bb = ac_exp(mk - ms);
            l = l * a + sP[k][rl][1] * bb;
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] = acc[d] * a + sP[k][rl][2 + d] * bb;
            m = mx;
        }
        float* o = out + i * os_seq + b * os_b + HD * h;
        const float inv = 1.0f / l;                                  // l == 0 (every column -inf): 0 * inf = NaN, as torch's softmax
#pragma unroll
        for (int d = 0; d < HD; ++d) o[d] = acc[d] * inv;
        if (wmax) {
            wmax[((size_t)b * 8 + h) * rows + i] = m;
            wsum[((size_t)b * 8 + h) * rows + i] = l;
        }
    }
}

// head-averaged weights w[b][i][j] = 1/8 sum_h exp(s_hij - max_hi) / sum_hi from the forward's per-(slot, head, row) maximum and sum
template <int MODE, bool MASKED>
__global__ __launch_bounds__(256) void attn_core_weights_kernel(const float* __restrict__ R, const float* __restrict__ C,
                                                                const float* __restrict__ mask, long ld_mask, const float* __restrict__ wmax,
                                                                const float* __restrict__ wsum, float* __restrict__ wout, int rows, int cols,
                                                                int Nb, long rs_seq, long rs_b, long cs_seq, long cs_b, float rscale,
                                                                float cscale) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)Nb * rows * cols) return;
    const int j = idx % cols, i = (idx / cols) % rows, b = idx / ((long)cols * rows);
    const float mk = MASKED ? mask[(long)i * ld_mask + j] : 0.f;
    float s = 0.f;
    for (int h = 0; h < 8; ++h) {
        float rr[AC_HD], cc[AC_HD];
        ac_load<MODE>(R + i * rs_seq + b * rs_b + AC_HD * h, rscale, rr);
        ac_load<MODE>(C + j * cs_seq + b * cs_b + AC_HD * h, cscale, cc);
        float dot = rr[0] * cc[0];
#pragma unroll
        for (int d = 1; d < AC_HD; ++d) dot = fmaf(rr[d], cc[d], dot);
        const size_t e = ((size_t)b * 8 + h) * rows + i;
        s += ac_exp(ac_score<MODE>(dot) + mk - wmax[e]) / wsum[e];   // a fully masked row: -inf - -inf = NaN, as its output row
    }
    wout[idx] = s * 0.125f;
}

// ---------------------------------------------------------------------------------------------------
// Backward, on the plan of train_attn.hip's attn_rc_bwd_kernel: one workgroup per (slot, head) owns all rows and columns, operands in LDS, no
// atomics, fixed summation order; the outputs are overwritten.  rho = rscale R[r], gam = cscale C[c];
//   P = softmax_c(s + mask), dP = dO[r] . V[c], dS = P (dP - sum_c' P dP), dV[c] = sum_r P dO[r];
//   mode 1: s = rho . gam,               dR[r] = rscale sum_c dS gam_c,  dC[c] = cscale sum_r dS rho_r
//   mode 0: s = -acos(x), x = clamp(rho^ . gam^): g = dS / sqrt(1 - x^2) where the clamp did not bind (torch.clamp: bounds inclusive), else 0;
//           dR[r] = rscale / |rho| (drho^ - rho^ (rho^ . drho^)), drho^ = sum_c g gam^_c  (dC likewise)
// A position masked with -inf has P = 0 and contributes nothing; the mask gets no gradient.  Pass 1 (thread = row) finds the row's maximum
// first (skipped for unmasked geodesic scores, which are <= 0), pass 2 (thread = column) reads it back from LDS.
// LDS: rows (2 HD + 3) + cols 2 HD floats.
// ---------------------------------------------------------------------------------------------------
#define AC_BWD_LDS_BYTES (64 * 1024)
template <int MODE, bool MASKED>
__global__ __launch_bounds__(256) void attn_core_bwd_kernel(const float* __restrict__ R, const float* __restrict__ C, const float* __restrict__ V,
                                                            const float* __restrict__ mask, long ld_mask, const float* __restrict__ dO,
                                                            float* __restrict__ dR, float* __restrict__ dC, float* __restrict__ dV, int rows,
                                                            int cols, long rs_seq, long rs_b, long cs_seq, long cs_b, long vs_seq, long vs_b,
                                                            long os_seq, long os_b, float rscale, float cscale) {
    constexpr int HD = AC_HD;
    extern __shared__ float ac_sm[];
    float* rh = ac_sm;              // [rows][HD] rho (mode 0: rho^)
    float* dd = rh + rows * HD;     // [rows][HD] dO
    float* rmax = dd + rows * HD;   // [rows] max_c (s + mask)
    float* rinv = rmax + rows;      // [rows] 1 / sum_c exp
    float* rdot = rinv + rows;      // [rows] sum_c P dP
    float* ch = rdot + rows;        // [cols][HD] gam (mode 0: gam^)
    float* vv = ch + cols * HD;     // [cols][HD] V
    const int b = blockIdx.x / 8, h = blockIdx.x % 8;
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        float x[HD];
        ac_load<MODE>(R + r * rs_seq + b * rs_b + HD * h, rscale, x);
        const float* po = dO + r * os_seq + b * os_b + HD * h;
#pragma unroll
        for (int d = 0; d < HD; ++d) { rh[r * HD + d] = x[d]; dd[r * HD + d] = po[d]; }
    }
    for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        float x[HD];
        ac_load<MODE>(C + c * cs_seq + b * cs_b + HD * h, cscale, x);
        const float* pv = V + c * vs_seq + b * vs_b + HD * h;
#pragma unroll
        for (int d = 0; d < HD; ++d) { ch[c * HD + d] = x[d]; vv[c * HD + d] = pv[d]; }
    }
    __syncthreads();
    const float lo = -1.0f + 1e-4f, hi = 1.0f - 1e-4f;
    // pass 1 (thread = row r): maximum, softmax denominator, sum_c P dP, dR[r]
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        const float* mrow = MASKED ? mask + (long)r * ld_mask : nullptr;
        float mx = 0.f;
        if (MODE == 1 || MASKED) {
            mx = AC_NINF;
            for (int c = 0; c < cols; ++c) {
                float dot = 0.f;
#pragma unroll
                for (int d = 0; d < HD; ++d) dot += rh[r * HD + d] * ch[c * HD + d];
                float s = MODE == 0 ? -acosf(fminf(fmaxf(dot, lo), hi)) : dot;
                if (MASKED) s += mrow[c];
                mx = fmaxf(mx, s);
            }
        }
        float se = 0.f, sp = 0.f;
        for (int c = 0; c < cols; ++c) {
            float dot = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { dot += rh[r * HD + d] * ch[c * HD + d]; dp += dd[r * HD + d] * vv[c * HD + d]; }
            float s = MODE == 0 ? -acosf(fminf(fmaxf(dot, lo), hi)) : dot;
            if (MASKED) s += mrow[c];
            const float ex = expf(s - mx);
            se += ex;
            sp += ex * dp;
        }
        const float ri = 1.0f / se, rd = sp / se;
        rmax[r] = mx;
        rinv[r] = ri;
        rdot[r] = rd;
        float g[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) g[d] = 0.f;
        for (int c = 0; c < cols; ++c) {
            float dot = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { dot += rh[r * HD + d] * ch[c * HD + d]; dp += dd[r * HD + d] * vv[c * HD + d]; }
            const float cl = fminf(fmaxf(dot, lo), hi);
            float s = MODE == 0 ? -acosf(cl) : dot;
            if (MASKED) s += mrow[c];
            const float dS = expf(s - mx) * ri * (dp - rd);
            float gs = dS;
            if (MODE == 0) gs = (dot >= lo && dot <= hi) ? dS / sqrtf(1.0f - cl * cl) : 0.f;   // d(-acos x)/dx = 1/sqrt(1-x^2)
#pragma unroll
            for (int d = 0; d < HD; ++d) g[d] += gs * ch[c * HD + d];
        }
        float* o = dR + r * rs_seq + b * rs_b + HD * h;
        if (MODE == 0) {
            const float* p = R + r * rs_seq + b * rs_b + HD * h;
            float ss = 0.f, pr = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { const float x = p[d] * rscale; ss += x * x; pr += g[d] * rh[r * HD + d]; }
            const float rn = rscale / sqrtf(ss);
#pragma unroll
            for (int d = 0; d < HD; ++d) o[d] = (g[d] - rh[r * HD + d] * pr) * rn;
        } else {
#pragma unroll
            for (int d = 0; d < HD; ++d) o[d] = g[d] * rscale;
        }
    }
    __syncthreads();
    // pass 2 (thread = column c): dC[c], dV[c]; lanes walk a mask row together (coalesced)
    for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        float g[HD], dv[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) g[d] = dv[d] = 0.f;
        for (int r = 0; r < rows; ++r) {
            float dot = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { dot += rh[r * HD + d] * ch[c * HD + d]; dp += dd[r * HD + d] * vv[c * HD + d]; }
            const float cl = fminf(fmaxf(dot, lo), hi);
            float s = MODE == 0 ? -acosf(cl) : dot;
            if (MASKED) s += mask[(long)r * ld_mask + c];
            const float P = expf(s - rmax[r]) * rinv[r];
            const float dS = P * (dp - rdot[r]);
            float gs = dS;
            if (MODE == 0) gs = (dot >= lo && dot <= hi) ? dS / sqrtf(1.0f - cl * cl) : 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { g[d] += gs * rh[r * HD + d]; dv[d] += P * dd[r * HD + d]; }
        }
        float* o = dC + c * cs_seq + b * cs_b + HD * h;
        float* ov = dV + c * vs_seq + b * vs_b + HD * h;
        if (MODE == 0) {
            const float* p = C + c * cs_seq + b * cs_b + HD * h;
            float ss = 0.f, pr = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { const float x = p[d] * cscale; ss += x * x; pr += g[d] * ch[c * HD + d]; }
            const float cn = cscale / sqrtf(ss);
#pragma unroll
            for (int d = 0; d < HD; ++d) o[d] = (g[d] - ch[c * HD + d] * pr) * cn;
        } else {
#pragma unroll
            for (int d = 0; d < HD; ++d) o[d] = g[d] * cscale;
        }
#pragma unroll
        for (int d = 0; d < HD; ++d) ov[d] = dv[d];
    }
}

// ---------------------------------------------------------------------------------------------------
extern "C" int sttode_attn_core(const float* R, const float* C, const float* V, const float* mask, long ld_mask, float* out, float* wmax,
                                float* wsum, float* wout, int rows, int cols, int Nb, long rs_seq, long rs_b, long cs_seq, long cs_b,
                                long vs_seq, long vs_b, long os_seq, long os_b, float rscale, float cscale, int mode, void* stream) {
    STT_REQUIRE(R && C && V && out, "sttode_attn_core: null pointer");
    STT_REQUIRE(rows > 0 && cols > 0 && Nb > 0 && Nb * 8L <= 65535, "sttode_attn_core: bad rows/cols/Nb (Nb*8 must fit gridDim.y)");
    STT_REQUIRE(mode == 0 || mode == 1, "sttode_attn_core: mode must be 0 (geodesic) or 1 (dot product)");
    STT_REQUIRE(!mask || ld_mask >= cols, "sttode_attn_core: ld_mask is smaller than cols");
    STT_REQUIRE((wmax != nullptr) == (wsum != nullptr), "sttode_attn_core: the max and sum workspaces come together");
    STT_REQUIRE(!wout || wmax, "sttode_attn_core: weights output needs the max and sum workspaces");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((rows + 63) / 64, Nb * 8);
    const long tot = (long)Nb * rows * cols;
    const dim3 wgrid((unsigned)((tot + 255) / 256));
#define AC_GO(MODE, MASKED)                                                                                                                  \
    do {                                                                                                                                     \
        hipLaunchKernelGGL((attn_core_kernel<MODE, MASKED>), grid, dim3(256), 0, s, R, C, V, mask, ld_mask, out, wmax, wsum, rows, cols, rs_seq, \
                           rs_b, cs_seq, cs_b, vs_seq, vs_b, os_seq, os_b, rscale, cscale);                                                  \
        if (wout)                                                                                                                            \
            hipLaunchKernelGGL((attn_core_weights_kernel<MODE, MASKED>), wgrid, dim3(256), 0, s, R, C, mask, ld_mask, wmax, wsum, wout, rows, \
                               cols, Nb, rs_seq, rs_b, cs_seq, cs_b, rscale, cscale);                                                        \
    } while (0)
    if (mode == 0) { if (mask) AC_GO(0, true); else AC_GO(0, false); }
    else { if (mask) AC_GO(1, true); else AC_GO(1, false); }
#undef AC_GO
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_attn_core_bwd(const float* R, const float* C, const float* V, const float* mask, long ld_mask, const float* dO, float* dR,
                                    float* dC, float* dV, int rows, int cols, int Nb, long rs_seq, long rs_b, long cs_seq, long cs_b,
                                    long vs_seq, long vs_b, long os_seq, long os_b, float rscale, float cscale, int mode, void* stream) {
    STT_REQUIRE(R && C && V && dO && dR && dC && dV, "sttode_attn_core_bwd: null pointer");
    STT_REQUIRE(rows > 0 && cols > 0 && Nb > 0 && Nb * 8L <= 65535, "sttode_attn_core_bwd: bad rows/cols/Nb (Nb*8 <= 65535)");
    STT_REQUIRE(mode == 0 || mode == 1, "sttode_attn_core_bwd: mode must be 0 (geodesic) or 1 (dot product)");
    STT_REQUIRE(!mask || ld_mask >= cols, "sttode_attn_core_bwd: ld_mask is smaller than cols");
    const size_t shm = ((size_t)rows * (2 * AC_HD + 3) + (size_t)cols * (2 * AC_HD)) * sizeof(float);
    STT_REQUIRE(shm <= AC_BWD_LDS_BYTES, "sttode_attn_core_bwd: rows x cols too large for the attention backward (rows (2 head_dim + 3) + "
                                         "cols 2 head_dim floats of LDS must fit 64 KiB)");
    const int mx = rows > cols ? rows : cols;
    const dim3 block(mx < 256 ? ((mx + 63) / 64) * 64 : 256);
    hipStream_t s = (hipStream_t)stream;
#define AC_GO(MODE, MASKED)                                                                                                                   \
    hipLaunchKernelGGL((attn_core_bwd_kernel<MODE, MASKED>), dim3(Nb * 8), block, shm, s, R, C, V, mask, ld_mask, dO, dR, dC, dV, rows, cols, \
                       rs_seq, rs_b, cs_seq, cs_b, vs_seq, vs_b, os_seq, os_b, rscale, cscale)
    if (mode == 0) { if (mask) AC_GO(0, true); else AC_GO(0, false); }
    else { if (mask) AC_GO(1, true); else AC_GO(1, false); }
#undef AC_GO
    STT_HIP(hipGetLastError());
    return 0;
}
