// Training step through a non-default ODE integrator: the stage combinations of the fixed-grid Runge-Kutta / multi-step Euler program and
// their adjoints (sttode_amd/odestages.py spells the program out, sttode_amd/training.py Engine._ode_* runs it).
//
// Reference: oracle.sttode_ref.ode_integrate_ref / hypertransformer.ode_integrate (uniform grid over [0, ode_time]; Euler, torchdiffeq's
// 3/8-rule 'rk4', the classical RK4), ode_demo.py:228 (relu of the final state).  Every piece of the program that is not the ODE function is a
// linear combination of row-major [rows, width] matrices:
//   forward   stage input  Y_i = y + h sum_j a_ij k_j,   step  y' = y + h sum_i b_i k_i,   encoder output relu(y_T)
//   backward  dk_i = h b_i dy' + h sum_{l > i} a_li dY_l,   dy = dy' + sum_i dY_i,   dy_T = dfeat * (y_T > 0)
// One launch combines up to STT_ODE_MAX_TERMS matrices for each of up to STT_ODE_MAX_JOBS jobs (the past and the future trunk side by side).
#include "api_util.hpp"
#include "ode_body.hpp"
#include "../../include/sttode_hip.h"

struct OdeCombineArgs {
    SttodeOdeCombine j[STT_ODE_MAX_JOBS];
    int width;
};

__global__ __launch_bounds__(256) void ode_combine_kernel(OdeCombineArgs a) {
    const SttodeOdeCombine& j = a.j[blockIdx.y];
    const long count = (long)j.rows * a.width;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (long)gridDim.x * blockDim.x) {
        const long r = e / a.width;
        const int c = (int)(e - r * a.width);
        float s = 0.f;
        for (int t = 0; t < j.nterms; ++t) s = fmaf(j.c[t], j.v[t][r * j.ld[t] + c], s);   // (terms in the caller's order)
        if (j.mask && !(j.mask[r * j.ld_mask + c] > 0.f)) s = 0.f;
        j.out[r * j.ld_out + c] = s;
        if (j.relu_out) j.relu_out[r * j.ld_relu + c] = fmaxf(s, 0.f);
    }
}

extern "C" int sttode_ode_combine(const void* jobs, int count, int width, void* stream) {
    STT_REQUIRE(jobs && count >= 1 && count <= STT_ODE_MAX_JOBS && width > 0, "sttode_ode_combine: null job table, bad job count or width");
    OdeCombineArgs a;
    a.width = width;
    long most = 0;
    for (int i = 0; i < count; ++i) {
        const SttodeOdeCombine& j = static_cast<const SttodeOdeCombine*>(jobs)[i];
        STT_REQUIRE(j.out && j.rows > 0 && j.nterms >= 1 && j.nterms <= STT_ODE_MAX_TERMS && j.ld_out >= width,
                    "sttode_ode_combine: job without output, rows or terms");
        STT_REQUIRE(!j.mask || j.ld_mask >= width, "sttode_ode_combine: mask row stride smaller than width");
        STT_REQUIRE(!j.relu_out || j.ld_relu >= width, "sttode_ode_combine: relu output row stride smaller than width");
        for (int t = 0; t < j.nterms; ++t)
            STT_REQUIRE(j.v[t] && j.ld[t] >= width, "sttode_ode_combine: null term or term row stride smaller than width");
        a.j[i] = j;
        const long c = (long)j.rows * width;
        most = c > most ? c : most;
    }
    long blocks = (most + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(ode_combine_kernel, dim3((unsigned)blocks, count), dim3(256), 0, (hipStream_t)stream, a);
    STT_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Per-stage dX chain (attention length 1): one launch per stage for both trunks.  A workgroup owns 16 rows: it recomputes f from the
// stage input (ode_body.hpp ode_f, the tape it needs stays in registers), forms dk from the stage-combination adjoint's terms (prologue),
// walks f backward to dY, and on a step's first stage also forms the gradient wrt the step's start state (epilogue).  Every linear
// layer's X and dY columns go to the chunk buffers of the deferred weight-gradient pass: no cross-row reduction here.
struct OdeBwdArgs {
    SttodeOdeStageBwd j[2];
};

static __device__ __forceinline__ f32x4 ode_terms(const SttodeOdeCombine& t, long row, int f, f32x4 acc) {
#pragma unroll
    for (int i = 0; i < STT_ODE_MAX_TERMS; ++i) {             // (constant indices into the kernel arguments)
        if (i >= t.nterms) break;
        const float* p = t.v[i] + row * t.ld[i] + f;
        acc[0] = fmaf(t.c[i], p[0], acc[0]); acc[1] = fmaf(t.c[i], p[1], acc[1]);
        acc[2] = fmaf(t.c[i], p[2], acc[2]); acc[3] = fmaf(t.c[i], p[3], acc[3]);
    }
    return acc;
}

__global__ __launch_bounds__(256) void ode_stage_bwd_kernel(OdeBwdArgs args) {
    const SttodeOdeStageBwd& J = blockIdx.y ? args.j[1] : args.j[0];   // (no dynamic index into the kernel arguments: no scratch copy)
    const int n = J.n, tile = blockIdx.x;
    if (tile * 16 >= n) return;                               // (uniform) the other trunk has more tiles
    __shared__ f32x4 sX[16 * 64];
    const int lane = threadIdx.x & 63, q = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = tile * 16 + (lane & 15);
    const bool live = col < n;
    const long cc = live ? col : n - 1;
    const int fo = 16 * w + 4 * q;                            // the lane's features in row tile w
    const OdeW W = {J.w[0], J.w[1], J.w[2], J.w[3], J.w[4], J.w[5], J.w[6], J.w[7], J.w[8], J.w[9], J.w[10], J.w[11], J.w[12], J.w[13],
                    J.w[14], J.w[15]};
    f32x4 Y[4], k[4];
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk) Y[Tk] = ld4(J.y + cc * 64 + 16 * Tk + 4 * q);
    OdeAct A;
    ode_f(W, Y, sX, w, lane, q, live, J.f1 + cc * 1024, k, A);
    if (live) {
        st4(J.attn + cc * 64 + fo, A.v);
        st4(J.ao + cc * 64 + fo, A.ao);
        st4(J.h + cc * 64 + fo, ode_pick(A.h, w));
    }
    // prologue: dk = h b_i dy' + h sum_{l > i} a_li dY_l (the terms the caller lists)
    f32x4 dk[4];
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk) dk[Tk] = ode_terms(J.kb, cc, 16 * Tk + 4 * q, splat4(0.f));
    // ---- LN2
    f32x4 ds2[4];
    ode_ln_bwd(dk, A.xh2, A.rs2, W.ln2w, ds2, q);
    if (live) {
        st4(J.dsum2 + cc * 64 + fo, ode_pick(ds2, w));
        st4(J.ln + cc * 256 + fo, ode_pick(dk, w) * ode_pick(A.xh2, w));
        st4(J.ln + cc * 256 + 64 + fo, ode_pick(dk, w));
    }
    // ---- FFN: df1 = (W2^T ds2) * (W1 h + b1 > 0) per hidden tile of the wave, dh = ds2 + W1^T df1 (partial sums over the waves' tiles)
    f32x4 dhp[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) dhp[it] = splat4(0.f);
#pragma unroll 1
    for (int i = 0; i < 16; ++i) {
        const int hn = 4 * i + w;
        f32x4 pre = ld4(W.l1b + 16 * hn + 4 * q), d = splat4(0.f);
#pragma unroll
        for (int Tk = 0; Tk < 4; ++Tk) {
            pre = mfma_k16(pre, ode_wfrag(W.l1w, 64, hn, Tk, lane), A.h[Tk]);
            d = mfma_k16(d, ode_wfragT(W.l2w, 1024, hn, Tk, lane), ds2[Tk]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = pre[r] > 0.f ? d[r] : 0.f;
        if (live) st4(J.df1 + cc * 1024 + 16 * hn + 4 * q, d);
#pragma unroll
        for (int it = 0; it < 4; ++it) dhp[it] = mfma_k16(dhp[it], ode_wfragT(W.l1w, 64, it, hn, lane), d);
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) sX[(w * 4 + it) * 64 + lane] = dhp[it];   // (ode_f ended behind a barrier)
    __syncthreads();
    f32x4 dh[4];
#pragma unroll
    for (int it = 0; it < 4; ++it)
        dh[it] = ds2[it] + (((sX[(0 * 4 + it) * 64 + lane] + sX[(1 * 4 + it) * 64 + lane]) + sX[(2 * 4 + it) * 64 + lane]) + sX[(3 * 4 + it) * 64 + lane]);
    __syncthreads();
    // ---- LN1, then the gate (row tile w)
    f32x4 d1[4];
    ode_ln_bwd(dh, A.xh1, A.rs1, W.ln1w, d1, q);
    const f32x4 d1w = ode_pick(d1, w);
    f32x4 du, dv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        du[r] = d1w[r] * A.ss[r] * (1.0f - A.tt[r] * A.tt[r]);
        dv[r] = d1w[r] * A.tt[r] * A.ss[r] * (1.0f - A.ss[r]);
    }
    if (live) {
        st4(J.ln + cc * 256 + 128 + fo, ode_pick(dh, w) * ode_pick(A.xh1, w));
        st4(J.ln + cc * 256 + 192 + fo, ode_pick(dh, w));
        st4(J.du + cc * 64 + fo, du);
        st4(J.dv + cc * 64 + fo, dv);
    }
    sX[(0 * 4 + w) * 64 + lane] = du;
    sX[(1 * 4 + w) * 64 + lane] = dv;
    __syncthreads();
    // ---- dao = Wi^T du + Wg^T dv, dattn = Wo^T dao, dY = d1 + Wv^T dattn
    f32x4 dao = splat4(0.f);
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk) {
        dao = mfma_k16(dao, ode_wfragT(W.infow, 64, w, Tk, lane), sX[(0 * 4 + Tk) * 64 + lane]);
        dao = mfma_k16(dao, ode_wfragT(W.gatew, 64, w, Tk, lane), sX[(1 * 4 + Tk) * 64 + lane]);
    }
    if (live) st4(J.dao + cc * 64 + fo, dao);
    sX[(2 * 4 + w) * 64 + lane] = dao;
    __syncthreads();
    f32x4 da = splat4(0.f);
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk) da = mfma_k16(da, ode_wfragT(W.outw, 64, w, Tk, lane), sX[(2 * 4 + Tk) * 64 + lane]);
    if (live) st4(J.dattn + cc * 64 + fo, da);
    sX[(3 * 4 + w) * 64 + lane] = da;
    __syncthreads();
    f32x4 dY = d1w;
#pragma unroll
    for (int Tk = 0; Tk < 4; ++Tk) dY = mfma_k16(dY, ode_wfragT(W.inw + 128 * 64, 64, w, Tk, lane), sX[(3 * 4 + Tk) * 64 + lane]);
    // epilogue: the stage's input gradient, and on a step's first stage the gradient wrt the step's start state
    if (live) {
        st4(J.dy + cc * 64 + fo, dY);
        if (J.next.out) st4(J.next.out + cc * J.next.ld_out + fo, ode_terms(J.next, cc, fo, dY));
    }
}

static bool ode_terms_ok(const SttodeOdeCombine& t, int min_terms) {
    if (t.nterms < min_terms || t.nterms > STT_ODE_MAX_TERMS) return false;
    for (int i = 0; i < t.nterms; ++i)
        if (!t.v[i] || t.ld[i] < 64) return false;
    return true;
}

extern "C" int sttode_ode_stage_bwd(const void* jobs, int count, void* stream) {
    STT_REQUIRE(jobs && count >= 1 && count <= 2, "sttode_ode_stage_bwd: null job table or job count not 1..2");
    OdeBwdArgs a = {};
    int tiles = 0;
    for (int i = 0; i < count; ++i) {
        const SttodeOdeStageBwd& j = static_cast<const SttodeOdeStageBwd*>(jobs)[i];
        bool ok = j.n > 0 && j.y && j.dy && j.attn && j.ao && j.h && j.f1 && j.dsum2 && j.df1 && j.du && j.dv && j.dao && j.dattn && j.ln;
        for (int k = 0; k < 16; ++k) ok = ok && j.w[k];
        STT_REQUIRE(ok, "sttode_ode_stage_bwd: null pointer or no rows in a job");
        STT_REQUIRE(ode_terms_ok(j.kb, 1) && (!j.next.out || (ode_terms_ok(j.next, 0) && j.next.ld_out >= 64)),
                    "sttode_ode_stage_bwd: bad combination terms");
        a.j[i] = j;
        const int t = (j.n + 15) / 16;
        tiles = t > tiles ? t : tiles;
    }
    hipLaunchKernelGGL(ode_stage_bwd_kernel, dim3(tiles, count), dim3(256), 0, (hipStream_t)stream, a);
    STT_HIP(hipGetLastError());
    return 0;
}
