// Training step, the recurrent and convolutional pieces (family index: train.hip): GRU cell forward / backward, the whole GRU sequence
// in one launch (two sizes) and conv1d k = 3 forward / backward.
#include "api_util.hpp"
#include "chain.hpp"

// ---------------------------------------------------------------------------------------------------
// GRU cell (torch.nn.GRU gate order r | z | n, model/STTODE.py:68): gi = W_ih e_t + b_ih (rows m*Tp + t), gh = W_hh h + b_hh
//   r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r * gh_n), h' = (1 - z) * n + z * h
// tape per step: r, z, n, gh_n  [m, 4*96]
// ---------------------------------------------------------------------------------------------------
__global__ void gru_cell_fwd_kernel(const float* gi, long ldgi, const float* gh, const float* hprev, float* hnew, float* tape, int m) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)m * 96) return;
    const int c = (int)(e / 96), f = (int)(e % 96);
    const float* gic = gi + (long)c * ldgi;
    const float* ghc = gh + (long)c * 288;
    const float r = 1.0f / (1.0f + expf(-(gic[f] + ghc[f])));
    const float z = 1.0f / (1.0f + expf(-(gic[96 + f] + ghc[96 + f])));
    const float hn = ghc[192 + f];
    const float n = tanhf(gic[192 + f] + r * hn);
    const float hp = hprev ? hprev[e] : 0.f;
    hnew[e] = (1.0f - z) * n + z * hp;
    float* t = tape + (long)c * 384;
    t[f] = r; t[96 + f] = z; t[192 + f] = n; t[288 + f] = hn;
}
// dh: grad wrt h' (in) ; writes dgi [m, 288] (rows with ld ldgi), dgh [m, 288], dhprev = dh * z (out, overwrites)
__global__ void gru_cell_bwd_kernel(const float* dh, const float* tape, const float* hprev, float* dgi, long ldgi, float* dgh,
                                    float* dhprev, int m) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)m * 96) return;
    const int c = (int)(e / 96), f = (int)(e % 96);
    const float* t = tape + (long)c * 384;
    const float r = t[f], z = t[96 + f], n = t[192 + f], hn = t[288 + f];
    const float hp = hprev ? hprev[e] : 0.f;
    const float d = dh[e];
    const float dn = d * (1.0f - z), dz = d * (hp - n);
    const float dnp = dn * (1.0f - n * n);
    const float drp = dnp * hn * r * (1.0f - r);
    const float dzp = dz * z * (1.0f - z);
    float* gi = dgi + (long)c * ldgi;
    float* gh = dgh + (long)c * 288;
    gi[f] = drp; gi[96 + f] = dzp; gi[192 + f] = dnp;
    gh[f] = drp; gh[96 + f] = dzp; gh[192 + f] = dnp * r;
    dhprev[e] = d * z;
}
extern "C" int sttode_gru_cell_fwd(const float* gi, long ldgi, const float* gh, const float* hprev, float* hnew, float* tape, int m,
                                   void* stream) {
    STT_REQUIRE(gi && gh && hnew && tape && m > 0, "sttode_gru_cell_fwd: bad argument");
    const long tot = (long)m * 96;
    hipLaunchKernelGGL(gru_cell_fwd_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gi, ldgi, gh, hprev, hnew, tape, m);
    STT_HIP(hipGetLastError());
    return 0;
}
extern "C" int sttode_gru_cell_bwd(const float* dh, const float* tape, const float* hprev, float* dgi, long ldgi, float* dgh,
                                   float* dhprev, int m, void* stream) {
    STT_REQUIRE(dh && tape && dgi && dgh && dhprev && m > 0, "sttode_gru_cell_bwd: bad argument");
    const long tot = (long)m * 96;
    hipLaunchKernelGGL(gru_cell_bwd_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dh, tape, hprev, dgi, ldgi, dgh, dhprev, m);
    STT_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Whole-sequence GRU for the training step: columns are independent, so ONE launch runs all Tp steps (forward) or the whole
// BPTT (backward).  WG = 16 columns x 6 waves; wave j owns hidden features [16j, 16j+16) of all three gates.  The W_hh
// fragments a wave needs (18 f32x4 forward: rows of its 3 gate tiles; 18 backward: its 16 columns of W_hh as the A operand
// of dh_prev += dgh W_hh) stay in REGISTERS for all steps; h (forward) / dgh (backward) is exchanged through LDS once per step.
// ---------------------------------------------------------------------------------------------------
#define GSEQ_LDH 100   // padded row length of the h exchange buffer (floats)
#define GSEQ_LDG 292   // padded row length of the dgh exchange buffer

__global__ __launch_bounds__(384) void gru_seq_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ Whh,
                                                          const float* __restrict__ bhh, float* __restrict__ H,
                                                          float* __restrict__ tapes, float* __restrict__ hfinal, long ldhf, int m,
                                                          int Tp) {
    __shared__ float sH[16 * GSEQ_LDH];
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4, j = threadIdx.x >> 6;
    const int col = blockIdx.x * 16 + c;
    const bool ok = col < m;
    const int f = 16 * j + 4 * q;                       // first of this lane's 4 hidden features
    f32x4 w[3][6], bias[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
#pragma unroll
        for (int T = 0; T < 6; ++T) w[g][T] = ld4(Whh + (long)(g * 96 + 16 * j + c) * 96 + 16 * T + 4 * q);
        bias[g] = ld4(bhh + g * 96 + f);
    }
    for (int i = threadIdx.x; i < 16 * GSEQ_LDH; i += 384) sH[i] = 0.f;
    if (ok) st4(H + (long)col * 96 + f, splat4(0.f));   // H[0] = h_{-1} = 0: the backward pass reads it (the caller need not zero H)
    __syncthreads();
    // the input-gate rows of step t + 1 travel while step t runs (requested inside the step they cost an L2 round trip per step: 8 of them
    // were a third of the launch at scene sizes)
    const float* gic0 = gi + (long)(ok ? col : 0) * Tp * 288;
    f32x4 gr_n = ld4(gic0 + f), gz_n = ld4(gic0 + 96 + f), gn_n = ld4(gic0 + 192 + f);
    for (int t = 0; t < Tp; ++t) {
        const f32x4 gr = gr_n, gz = gz_n, gn = gn_n;
        if (t + 1 < Tp) {
            const float* gn1 = gic0 + (long)(t + 1) * 288;
            gr_n = ld4(gn1 + f); gz_n = ld4(gn1 + 96 + f); gn_n = ld4(gn1 + 192 + f);
        }
        f32x4 acc[3] = {bias[0], bias[1], bias[2]};
#pragma unroll
        for (int T = 0; T < 6; ++T) {
            const f32x4 b = ld4(sH + c * GSEQ_LDH + 16 * T + 4 * q);
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] = mfma_k16(acc[g], w[g][T], b);
        }
        const f32x4 hp = ld4(sH + c * GSEQ_LDH + f);
        f32x4 hn = hp;
        if (ok) {
            f32x4 r, z, n;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // (the hardware's exp2 / rcp forms of chain.hpp, as in the inference GRU: absolute error ~1e-7; expf / tanhf / IEEE division
                // were ~1 500 vector instructions per lane and step -- most of a 4.7-us step at scene sizes)
                r[e] = sigmoidf_(gr[e] + acc[0][e]);
                z[e] = sigmoidf_(gz[e] + acc[1][e]);
                n[e] = tanhf_(gn[e] + r[e] * acc[2][e]);
                hn[e] = (1.0f - z[e]) * n[e] + z[e] * hp[e];
            }
            float* tp = tapes + ((long)t * m + col) * 384;
            st4(tp + f, r); st4(tp + 96 + f, z); st4(tp + 192 + f, n); st4(tp + 288 + f, acc[2]);
            st4(H + ((long)(t + 1) * m + col) * 96 + f, hn);
            if (hfinal && t == Tp - 1) st4(hfinal + (long)col * ldhf + f, hn);
        }
        __syncthreads();                                // every wave has read h_{t-1}
        st4(sH + c * GSEQ_LDH + f, hn);
        __syncthreads();
    }
}

__global__ __launch_bounds__(384) void gru_seq_bwd_kernel(const float* __restrict__ dh_last, long lddh, const float* __restrict__ tapes,
                                                          const float* __restrict__ H, const float* __restrict__ Whh,
                                                          float* __restrict__ dgi, float* __restrict__ dgh, int m, int Tp) {
    __shared__ float sG[16 * GSEQ_LDG];
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4, j = threadIdx.x >> 6;
    const int col = blockIdx.x * 16 + c;
    const bool ok = col < m;
    const int f = 16 * j + 4 * q;
    // A operand of dh_prev[:, 16j..16j+16) += dgh W_hh[:, 16j..]:  A[i = 16j + c][k] = W_hh[k][16j + c], k = 16T + 4q + r
    f32x4 w[18];
#pragma unroll
    for (int T = 0; T < 18; ++T)
#pragma unroll
        for (int r = 0; r < 4; ++r) w[T][r] = Whh[(long)(16 * T + 4 * q + r) * 96 + 16 * j + c];
    f32x4 dh = ok ? ld4(dh_last + (long)col * lddh + f) : splat4(0.f);
    // (requesting the tape of step t - 1 during step t, as the forward launch does with its rows, was measured: the same 30 us at scene
    // sizes and 47 -> 55 us at NBA size -- five more live f32x4 per lane)
    for (int t = Tp - 1; t >= 0; --t) {
        f32x4 dr = splat4(0.f), dz = dr, dn = dr, dhn = dr, dhz = dr;
        f32x4 r = dr, z = dr, n = dr, hn = dr, hp = dr;
        if (ok) {
            const float* tp = tapes + ((long)t * m + col) * 384;
            r = ld4(tp + f); z = ld4(tp + 96 + f); n = ld4(tp + 192 + f); hn = ld4(tp + 288 + f);
            hp = ld4(H + ((long)t * m + col) * 96 + f);
        }
        if (ok) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = dh[e];
                const float dnp = d * (1.0f - z[e]) * (1.0f - n[e] * n[e]);
                dn[e] = dnp;
                dr[e] = dnp * hn[e] * r[e] * (1.0f - r[e]);
                dz[e] = d * (hp[e] - n[e]) * z[e] * (1.0f - z[e]);
                dhn[e] = dnp * r[e];
                dhz[e] = d * z[e];
            }
            float* gi = dgi + ((long)col * Tp + t) * 288;
            st4(gi + f, dr); st4(gi + 96 + f, dz); st4(gi + 192 + f, dn);
            float* gh = dgh + ((long)t * m + col) * 288;
            st4(gh + f, dr); st4(gh + 96 + f, dz); st4(gh + 192 + f, dhn);
        }
        st4(sG + c * GSEQ_LDG + f, dr);
        st4(sG + c * GSEQ_LDG + 96 + f, dz);
        st4(sG + c * GSEQ_LDG + 192 + f, dhn);
        __syncthreads();
        f32x4 acc = dhz;
#pragma unroll
        for (int T = 0; T < 18; ++T) acc = mfma_k16(acc, w[T], ld4(sG + c * GSEQ_LDG + 16 * T + 4 * q));
        dh = acc;
        __syncthreads();                                // sG is rewritten by the next step
    }
}

// ---------------------------------------------------------------------------------------------------
// The same two launches for FEW columns (round 5; m <= GSEQ_SMALL_MAX = 1024: one scene per step, the live columns of a backward
// pass, the per-agent first block).  The kernels above put 16 columns on a 16-wide MFMA tile and all of a tile's W_hh products on ONE CU:
// 885 kFLOP per step = 1.4-1.9 us of that CU's matrix pipe per step of the recurrence, whatever m is -- with m = 32 columns two CUs work
// and 254 idle, 28-33 us per launch, four launches per training step (20 % of a one-scene step).  Here a workgroup owns FOUR columns and
// the products run on the vector ALUs with the weight row (forward: W_hh[row][0..95]; backward: 72 of W_hh[..][f]'s 288) in registers and
// h / the gate gradients broadcast from LDS: 4x more workgroups, ~0.5 us per step.  Same tape layout, same arithmetic per element; the
// 96- / 288-term sums run as four interleaved partial sums instead of the MFMA's blocked order (differences at fp32 rounding).
// ---------------------------------------------------------------------------------------------------
#define GSEQ_SC 4
__global__ __launch_bounds__(384) void gru_seq_fwd_small_kernel(const float* __restrict__ gi, const float* __restrict__ Whh,
                                                                const float* __restrict__ bhh, float* __restrict__ H,
                                                                float* __restrict__ tapes, float* __restrict__ hfinal, long ldhf, int m,
                                                                int Tp) {
    __shared__ __attribute__((aligned(16))) float sH[GSEQ_SC][96];
    __shared__ float sA[GSEQ_SC][288];
    const int tid = threadIdx.x;
    const bool mv = tid < 288;                       // matvec thread: one row of W_hh
    float w[96];
    float bias = 0.f;
    if (mv) {
#pragma unroll
        for (int k = 0; k < 24; ++k) {
            const f32x4 v = ld4(Whh + (long)tid * 96 + 4 * k);
            w[4 * k] = v[0]; w[4 * k + 1] = v[1]; w[4 * k + 2] = v[2]; w[4 * k + 3] = v[3];
        }
        bias = bhh[tid];
    } else {
#pragma unroll
        for (int k = 0; k < 96; ++k) w[k] = 0.f;
    }
    const int c = tid / 96, f = tid % 96;            // gate thread: (column, feature)
    const int col = blockIdx.x * GSEQ_SC + c;
    const bool ok = col < m;
    sH[c][f] = 0.f;
    if (ok) H[(long)col * 96 + f] = 0.f;             // H[0] = h_{-1} = 0: the backward pass reads it
    __syncthreads();
    const float* gic = gi + (long)(ok ? col : 0) * Tp * 288;
    for (int t = 0; t < Tp; ++t) {
        const float gr = gic[(long)t * 288 + f], gz = gic[(long)t * 288 + 96 + f], gn = gic[(long)t * 288 + 192 + f];   // (in flight under the products)
        if (mv) {
            f32x4 acc[GSEQ_SC];                       // four partial sums per column (k mod 4): short dependency chains, blocked like the MFMA's sums
#pragma unroll
            for (int cc = 0; cc < GSEQ_SC; ++cc) acc[cc] = splat4(0.f);
#pragma unroll
            for (int k = 0; k < 24; ++k) {
#pragma unroll
                for (int cc = 0; cc < GSEQ_SC; ++cc) {
                    const f32x4 h4 = *reinterpret_cast<const f32x4*>(&sH[cc][4 * k]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[cc][e] = fmaf(w[4 * k + e], h4[e], acc[cc][e]);
                }
            }
#pragma unroll
            for (int cc = 0; cc < GSEQ_SC; ++cc) sA[cc][tid] = bias + ((acc[cc][0] + acc[cc][1]) + (acc[cc][2] + acc[cc][3]));
        }
        __syncthreads();
        const float a2 = sA[c][192 + f], hp = sH[c][f];
        const float r = sigmoidf_(gr + sA[c][f]);
        const float z = sigmoidf_(gz + sA[c][96 + f]);
        const float n = tanhf_(gn + r * a2);
        const float hn = (1.0f - z) * n + z * hp;
        if (ok) {
            float* tp = tapes + ((long)t * m + col) * 384;
            tp[f] = r; tp[96 + f] = z; tp[192 + f] = n; tp[288 + f] = a2;
            H[((long)(t + 1) * m + col) * 96 + f] = hn;
            if (hfinal && t == Tp - 1) hfinal[(long)col * ldhf + f] = hn;
        }
        sH[c][f] = ok ? hn : 0.f;
        __syncthreads();
    }
}
__global__ __launch_bounds__(384) void gru_seq_bwd_small_kernel(const float* __restrict__ dh_last, long lddh, const float* __restrict__ tapes,
                                                                const float* __restrict__ H, const float* __restrict__ Whh,
                                                                float* __restrict__ dgi, float* __restrict__ dgh, int m, int Tp) {
    __shared__ __attribute__((aligned(16))) float sG[GSEQ_SC][288];   // (dr | dz | dhn) of the step
    __shared__ float sP[4][GSEQ_SC][96];                              // partial products of the four k ranges
    const int tid = threadIdx.x;
    const int c = tid / 96, f = tid % 96;            // element thread (column, feature); product thread (k range c, feature f)
    const int col = blockIdx.x * GSEQ_SC + c;
    const bool ok = col < m;
    float w[72];                                      // W_hh[72 c + k][f]: this thread's quarter of the 288-term sum for feature f
#pragma unroll
    for (int k = 0; k < 72; ++k) w[k] = Whh[(long)(72 * c + k) * 96 + f];
    float dh = ok ? dh_last[(long)col * lddh + f] : 0.f;
    for (int t = Tp - 1; t >= 0; --t) {
        float dr = 0.f, dz = 0.f, dn = 0.f, dhn = 0.f, dhz = 0.f;
        if (ok) {
            const float* tp = tapes + ((long)t * m + col) * 384;
            const float r = tp[f], z = tp[96 + f], n = tp[192 + f], hn = tp[288 + f];
            const float hp = H[((long)t * m + col) * 96 + f];
            const float dnp = dh * (1.0f - z) * (1.0f - n * n);
            dn = dnp;
            dr = dnp * hn * r * (1.0f - r);
            dz = dh * (hp - n) * z * (1.0f - z);
            dhn = dnp * r;
            dhz = dh * z;
            float* gi = dgi + ((long)col * Tp + t) * 288;
            gi[f] = dr; gi[96 + f] = dz; gi[192 + f] = dn;
            float* gh = dgh + ((long)t * m + col) * 288;
            gh[f] = dr; gh[96 + f] = dz; gh[192 + f] = dhn;
        }
        sG[c][f] = dr; sG[c][96 + f] = dz; sG[c][192 + f] = dhn;
        __syncthreads();
        f32x4 acc[GSEQ_SC];
#pragma unroll
        for (int cc = 0; cc < GSEQ_SC; ++cc) acc[cc] = splat4(0.f);
#pragma unroll
        for (int k = 0; k < 18; ++k) {
#pragma unroll
            for (int cc = 0; cc < GSEQ_SC; ++cc) {
                const f32x4 g4 = *reinterpret_cast<const f32x4*>(&sG[cc][72 * c + 4 * k]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[cc][e] = fmaf(g4[e], w[4 * k + e], acc[cc][e]);
            }
        }
#pragma unroll
        for (int cc = 0; cc < GSEQ_SC; ++cc) sP[c][cc][f] = (acc[cc][0] + acc[cc][1]) + (acc[cc][2] + acc[cc][3]);
        __syncthreads();
        dh = dhz + (((sP[0][c][f] + sP[1][c][f]) + sP[2][c][f]) + sP[3][c][f]);
        // (sG and sP are rewritten only after the next step's first barrier / this step's readers are past the second one)
    }
}
static constexpr int GSEQ_SMALL_MAX = 1024;   // columns up to which the few-column kernels above run (profiles/r05/train_gru_small_ab.txt)

extern "C" int sttode_gru_seq_fwd(const float* gi, const float* Whh, const float* bhh, float* H, float* tapes, float* hfinal,
                                  long ldhf, int m, int Tp, void* stream) {
    STT_REQUIRE(gi && Whh && bhh && H && tapes && m > 0 && Tp > 0, "sttode_gru_seq_fwd: bad argument");
    STT_REQUIRE(((size_t)Whh) % 16 == 0 && ((size_t)gi) % 16 == 0, "sttode_gru_seq_fwd: pointers must be 16-byte aligned");
    STT_REQUIRE(!hfinal || (((size_t)hfinal) % 16 == 0 && ldhf % 4 == 0 && ldhf >= 96), "sttode_gru_seq_fwd: hfinal must be 16-byte aligned rows of >= 96 floats");
    if (m <= GSEQ_SMALL_MAX)
        hipLaunchKernelGGL(gru_seq_fwd_small_kernel, dim3((m + GSEQ_SC - 1) / GSEQ_SC), dim3(384), 0, (hipStream_t)stream, gi, Whh, bhh, H, tapes, hfinal, ldhf, m, Tp);
    else
        hipLaunchKernelGGL(gru_seq_fwd_kernel, dim3((m + 15) / 16), dim3(384), 0, (hipStream_t)stream, gi, Whh, bhh, H, tapes, hfinal, ldhf, m, Tp);
    STT_HIP(hipGetLastError());
    return 0;
}
extern "C" int sttode_gru_seq_bwd(const float* dh_last, long lddh, const float* tapes, const float* H, const float* Whh, float* dgi,
                                  float* dgh, int m, int Tp, void* stream) {
    STT_REQUIRE(dh_last && tapes && H && Whh && dgi && dgh && m > 0 && Tp > 0, "sttode_gru_seq_bwd: bad argument");
    STT_REQUIRE(((size_t)dh_last) % 16 == 0 && lddh % 4 == 0 && lddh >= 96, "sttode_gru_seq_bwd: dh_last must be 16-byte aligned rows of >= 96 floats");
    if (m <= GSEQ_SMALL_MAX)
        hipLaunchKernelGGL(gru_seq_bwd_small_kernel, dim3((m + GSEQ_SC - 1) / GSEQ_SC), dim3(384), 0, (hipStream_t)stream, dh_last, lddh, tapes, H, Whh, dgi, dgh, m, Tp);
    else
        hipLaunchKernelGGL(gru_seq_bwd_kernel, dim3((m + 15) / 16), dim3(384), 0, (hipStream_t)stream, dh_last, lddh, tapes, H, Whh, dgi, dgh, m, Tp);
    STT_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// conv1d(2 -> 32, k = 3, pad = 1) + relu over x [m, T, 2] (model/STTODE.py:65); e [m, T, 32]
// x = xa[c / adiv] - (xb ? xb[c] : 0)   (x_true - x_hat of the previous block)
// ---------------------------------------------------------------------------------------------------
__global__ void conv_fwd_kernel(const float* xa, int adiv, const float* xb, const float* w, const float* b, float* x, float* e, int m, int T) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)m * T * 32) return;
    const int oc = (int)(id % 32), t = (int)((id / 32) % T), c = (int)(id / (32L * T));
    float acc = b[oc];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int tt = t + k - 1;
        if (tt < 0 || tt >= T) continue;
#pragma unroll
        for (int ic = 0; ic < 2; ++ic) {
            float v = xa[((long)(c / adiv) * T + tt) * 2 + ic];
            if (xb) v -= xb[((long)c * T + tt) * 2 + ic];
            acc += w[(oc * 2 + ic) * 3 + k] * v;
            if (oc == 0 && k == 1) x[((long)c * T + tt) * 2 + ic] = v;  // k == 1: tt == t, every (c, t) written once
        }
    }
    e[id] = fmaxf(acc, 0.f);
}
// de already masked by relu.  dx[c, t, ic] = sum_{oc,k} w[oc,ic,k] * de[c, t - k + 1, oc]
__global__ void conv_bwd_x_kernel(const float* de, const float* w, float* dx, int m, int T) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)m * T * 2) return;
    const int ic = (int)(id % 2), t = (int)((id / 2) % T), c = (int)(id / (2L * T));
    float acc = 0.f;
    for (int k = 0; k < 3; ++k) {
        const int te = t - k + 1;
        if (te < 0 || te >= T) continue;
        const float* d = de + ((long)c * T + te) * 32;
        for (int oc = 0; oc < 32; ++oc) acc += w[(oc * 2 + ic) * 3 + k] * d[oc];
    }
    dx[id] = acc;
}
// dW[oc,ic,k] += sum_{c,t} de[c,t,oc] * x[c,t+k-1,ic], db[oc] += sum de.  A WG walks a contiguous slab of (c,t) rows: thread
// (row lane 0..7, oc 0..31) reads de[row][oc] (one 128-byte line per row across the 32 oc threads) and the row's 3 x 2 inputs,
// keeps its 6 weight partials + 1 bias partial in registers, the 8 row lanes are combined through LDS and every WG writes one
// partial vector [224]; a second single-WG pass adds the partials in order (deterministic).
__global__ __launch_bounds__(256) void conv_bwd_w_kernel(const float* de, const float* x, float* part, int m, int T, int rows_per_wg, float* dw,
                                                         float* db) {   // dw != nullptr: ONE workgroup, its sums go straight into dw / db (no reduction launch)
    __shared__ float red[8][224];
    const int oc = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const long rows = (long)m * T;
    const long r0 = (long)blockIdx.x * rows_per_wg, r1 = min(r0 + rows_per_wg, rows);
    float w[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, b = 0.f;
    for (long r = r0 + rl; r < r1; r += 8) {
        const int t = (int)(r % T);
        const float d = de[r * 32 + oc];
        b += d;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int tt = t + k - 1;
            if (tt < 0 || tt >= T) continue;
            const float* xr = x + (r - t + tt) * 2;
            w[0 * 3 + k] += d * xr[0];
            w[1 * 3 + k] += d * xr[1];
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) red[rl][oc * 6 + j] = w[j];      // dw index = (oc*2 + ic)*3 + k = oc*6 + ic*3 + k
    red[rl][192 + oc] = b;
    __syncthreads();
    if (threadIdx.x < 224) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += red[i][threadIdx.x];
        if (dw) {
            if (threadIdx.x < 192) dw[threadIdx.x] += s;
            else db[threadIdx.x - 192] += s;
        } else {
            part[(long)blockIdx.x * 224 + threadIdx.x] = s;
        }
    }
}
// one wave per output j: lane l adds the partials g = l, l + 64, ... in order, then a fixed xor-shuffle tree (deterministic); a single
// 224-thread block walking up to 256 partials one after the other took 60 us at NBA batch sizes
__global__ __launch_bounds__(64) void conv_bwd_w_reduce_kernel(const float* part, int G, float* dw, float* db) {
    const int j = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int g = lane; g < G; g += 64) s += part[(long)g * 224 + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
        if (j < 192) dw[j] += s;
        else db[j - 192] += s;
    }
}
extern "C" int sttode_conv_fwd(const float* xa, int adiv, const float* xb, const float* w, const float* b, float* x, float* e, int m,
                               int T, void* stream) {
    STT_REQUIRE(xa && w && b && x && e && m > 0 && T > 0 && adiv > 0, "sttode_conv_fwd: bad argument");
    const long tot = (long)m * T * 32;
    hipLaunchKernelGGL(conv_fwd_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, xa, adiv, xb, w, b, x, e, m, T);
    STT_HIP(hipGetLastError());
    return 0;
}
extern "C" int sttode_conv_bwd(const float* de, const float* x, const float* w, float* dx, float* dw, float* db, int m, int T,
                               float* scratch, long scratch_floats, void* stream) {
    STT_REQUIRE(de && x && w && dw && db && scratch && m > 0 && T > 0, "sttode_conv_bwd: bad argument");
    const long rows = (long)m * T;
    int G = (int)((rows + 63) / 64);     // 8 rows per thread at scene sizes (512 per workgroup made an 11-workgroup launch of 43 us)
    if (G > 256) G = 256;
    STT_REQUIRE(scratch_floats >= (long)G * 224, "sttode_conv_bwd: scratch too small");   // (before any launch: a refused call writes nothing)
    if (dx) {
        const long tot = (long)m * T * 2;
        hipLaunchKernelGGL(conv_bwd_x_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, de, w, dx, m, T);
    }
    if (rows <= 128) {                   // very few rows (16 trips of the row loop): one workgroup adds into dw / db itself -- one launch, not two
        hipLaunchKernelGGL(conv_bwd_w_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, de, x, scratch, m, T, (int)rows, dw, db);
        STT_HIP(hipGetLastError());
        return 0;
    }
    const int rpw = (int)((rows + G - 1) / G);
    hipLaunchKernelGGL(conv_bwd_w_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, de, x, scratch, m, T, rpw, (float*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(conv_bwd_w_reduce_kernel, dim3(224), dim3(64), 0, (hipStream_t)stream, scratch, G, dw, db);
    STT_HIP(hipGetLastError());
    return 0;
}
