// The ODE function of the encoder trunk and its vector-Jacobian product for ONE 16-column tile, attention length 1 (scene batches): the
// device pieces of the non-default integrators' training kernels (train_trunk.hip ttrunk_ode_fwd_kernel, train_ode.hip ode_stage_bwd_kernel).
//
// f(Y) = LN2(h + W2 relu(W1 h + b1) + b2),  h = LN1(Y + tanh(Wi ao + bi) * sigmoid(Wg ao + bg)),  ao = Wo v + bo,  v = Wv Y + bv
// (hypertransformer.py:134-153; the softmax over one key is 1, so the attention output is v).
//
// Layout as in train_trunk.hip: a workgroup of 4 waves owns 16 columns (rows of the batch) on the MFMA lane columns; lane (c, q) of a
// full vector X[4] holds features 16 Tk + 4 q + 0..3 of column c in X[Tk]; wave w computes output row tile w of every 64-wide layer and
// hidden tiles w, w + 4, ... of the FFN; tiles are exchanged through the LDS slots sX[16][64].
#pragma once
#include "chain.hpp"

struct OdeW {
    const float *inw, *inb, *outw, *outb, *infow, *infob, *gatew, *gateb, *ln1w, *ln1b, *l1w, *l1b, *l2w, *l2b, *ln2w, *ln2b;
};

// A fragment (row tile it, k tile T) of a row-major W [I, ld]: lane (i, q) holds W[16 it + i][16 T + 4 q + 0..3]
__device__ __forceinline__ f32x4 ode_wfrag(const float* __restrict__ W, long ld, int it, int T, int lane) {
    return ld4(W + (long)(16 * it + (lane & 15)) * ld + 16 * T + 4 * (lane >> 4));
}
// ... of W^T (W [K, ld] row-major, the transposed product of a backward pass): lane (i, q) holds W[16 T + 4 q + r][16 it + i]
__device__ __forceinline__ f32x4 ode_wfragT(const float* __restrict__ W, long ld, int it, int T, int lane) {
    const float* p = W + (long)(16 * T + 4 * (lane >> 4)) * ld + 16 * it + (lane & 15);
    f32x4 r = {p[0], p[ld], p[2 * ld], p[3 * ld]};
    return r;
}
__device__ __forceinline__ f32x4 ode_pick(const f32x4 (&v)[4], int w) { return w == 0 ? v[0] : w == 1 ? v[1] : w == 2 ? v[2] : v[3]; }

// LayerNorm forward on a full vector: v <- gamma * xhat + beta; returns xhat and 1/std
__device__ __forceinline__ void ode_ln_fwd(f32x4 (&v)[4], const float* gamma, const float* beta, f32x4 (&xh)[4], float& rs, int q) {
    float s = 0.f;
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk) s += (v[Tk][0] + v[Tk][1]) + (v[Tk][2] + v[Tk][3]);
    const float mean = colsum_q(s) * (1.0f / 64.0f);
    float var = 0.f;
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk)
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float d = v[Tk][r] - mean; var += d * d; }
    rs = 1.0f / sqrtf(colsum_q(var) * (1.0f / 64.0f) + 1e-5f);
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk) {
        const f32x4 g = ld4(gamma + 16 * Tk + 4 * q), b = ld4(beta + 16 * Tk + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r) { xh[Tk][r] = (v[Tk][r] - mean) * rs; v[Tk][r] = xh[Tk][r] * g[r] + b[r]; }
    }
}
// LayerNorm backward on full vectors: dx = rs (dxh - mean(dxh) - xhat mean(dxh xhat)), dxh = dy gamma
__device__ __forceinline__ void ode_ln_bwd(const f32x4 (&dy)[4], const f32x4 (&xh)[4], float rs, const float* gamma, f32x4 (&dx)[4], int q) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk) {
        const f32x4 g = ld4(gamma + 16 * Tk + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r) { dx[Tk][r] = dy[Tk][r] * g[r]; s1 += dx[Tk][r]; s2 += dx[Tk][r] * xh[Tk][r]; }
    }
    const float m1 = colsum_q(s1) * (1.0f / 64.0f), m2 = colsum_q(s2) * (1.0f / 64.0f);
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk)
#pragma unroll
        for (int r = 0; r < 4; ++r) dx[Tk][r] = rs * (dx[Tk][r] - m1 - xh[Tk][r] * m2);
}

// What the VJP needs of a forward evaluation (kept in registers between the recompute and the backward walk)
struct OdeAct {
    f32x4 v, ao, tt, ss;          // own row tile w
    f32x4 h[4], xh1[4], xh2[4];   // full vectors
    float rs1, rs2;
};

// k = f(Y) (full vector) for the tile's columns.  f1 != nullptr: the hidden activation relu(W1 h + b1) of the lane's column is stored
// there (a row of 1024 floats) when `live`.  Every use of the slots sits between barriers, the first and the last included.
__device__ __forceinline__ void ode_f(const OdeW& W, const f32x4 (&Y)[4], f32x4* sX, int w, int lane, int q, bool live, float* f1,
                                      f32x4 (&k)[4], OdeAct& A) {
    A.v = ld4(W.inb + 128 + 16 * w + 4 * q);
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk) A.v = mfma_k16(A.v, ode_wfrag(W.inw, 64, 8 + w, Tk, lane), Y[Tk]);
    __syncthreads();
    sX[(2 * 4 + w) * 64 + lane] = A.v;
    __syncthreads();
    A.ao = ld4(W.outb + 16 * w + 4 * q);
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk) A.ao = mfma_k16(A.ao, ode_wfrag(W.outw, 64, w, Tk, lane), sX[(2 * 4 + Tk) * 64 + lane]);
    sX[(3 * 4 + w) * 64 + lane] = A.ao;
    __syncthreads();
    f32x4 vi = ld4(W.infob + 16 * w + 4 * q), vg = ld4(W.gateb + 16 * w + 4 * q);
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk) {
        const f32x4 o = sX[(3 * 4 + Tk) * 64 + lane];
        vi = mfma_k16(vi, ode_wfrag(W.infow, 64, w, Tk, lane), o);
        vg = mfma_k16(vg, ode_wfrag(W.gatew, 64, w, Tk, lane), o);
    }
    const f32x4 yw = ode_pick(Y, w);
    f32x4 s1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        A.tt[r] = tanhf(vi[r]);
        A.ss[r] = 1.0f / (1.0f + expf(-vg[r]));
        s1[r] = yw[r] + A.tt[r] * A.ss[r];
    }
    sX[(0 * 4 + w) * 64 + lane] = s1;
    __syncthreads();
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk) A.h[Tk] = sX[(0 * 4 + Tk) * 64 + lane];
    ode_ln_fwd(A.h, W.ln1w, W.ln1b, A.xh1, A.rs1, q);
    f32x4 ff[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) ff[it] = splat4(0.f);
#pragma unroll 1
    for (int i = 0; i < 16; ++i) {
        const int hn = 4 * i + w;
        f32x4 hid = ld4(W.l1b + 16 * hn + 4 * q);
#pragma unroll
        for (int Tk = 0; Tk < 4; ++Tk) hid = mfma_k16(hid, ode_wfrag(W.l1w, 64, hn, Tk, lane), A.h[Tk]);
        hid = relu4(hid);
        if (f1 && live) st4(f1 + 16 * hn + 4 * q, hid);
#pragma unroll
        for (int it = 0; it < 4; ++it) ff[it] = mfma_k16(ff[it], ode_wfrag(W.l2w, 1024, it, hn, lane), hid);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) sX[(w * 4 + it) * 64 + lane] = ff[it];
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const f32x4 tsum = ((sX[(0 * 4 + it) * 64 + lane] + sX[(1 * 4 + it) * 64 + lane]) + sX[(2 * 4 + it) * 64 + lane]) + sX[(3 * 4 + it) * 64 + lane];
        k[it] = A.h[it] + (tsum + ld4(W.l2b + 16 * it + 4 * q));
    }
    ode_ln_fwd(k, W.ln2w, W.ln2b, A.xh2, A.rs2, q);
    __syncthreads();
}
