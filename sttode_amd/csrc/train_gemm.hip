// Training step, the dense products (family index: train.hip).  The layers run on v_mfma_f32_16x16x4_f32 in the column-chain formulation
// of chain.hpp, as GENERIC kernels (any N / K, row-major nn.Parameter storage read in place, gradients accumulated straight into .grad
// storage), or above TGEMM_MIN_COLS / TGEMM_MIN_COLS_BWD columns on the LDS-tiled kernel (tgemm):
//   tlinear      out[c, i] = epi( sum_j in[c / xdiv, j] * Wop[i, j] )   Wop = W or W^T (input gradient)
//   twgrad       dW[n, k] += sum_c dY[c, n] * X[c / xdiv, k],  db[n] += sum_c dY[c, n]   (deterministic split + reduce)
// Device code first, then the host state of group mode (the queues g_red, g_grp, g_ts), their submit functions and the entry points.
// sttode_tgemm_group here is the one function that knows every queue of a group (train_group.hpp).
#include "api_util.hpp"
#include "chain.hpp"
#include "train_group.hpp"

// ---------------------------------------------------------------------------------------------------
// tlinear
// ---------------------------------------------------------------------------------------------------
struct TLin {
    const float* X; const float* W; const float* bias; const float* mask; float* Y;
    long ldx, ldw, ldy, ldm;
    int cols, J, I, trans, act, accumulate, xdiv, xvec, wvec, yvec;
    // what `accumulate` adds: row (col / adiv) of asrc -- Y itself (asrc = Y, adiv = 1: += into the output) or a per-GROUP table broadcast over
    // adiv consecutive columns (sttode_tlinear_tab: the decoder MLPs' per-agent layer-1 part W1[:, pf] pf + b1, shared by an agent's K samples)
    const float* asrc; long ldas; int adiv;
    int evec;   // I % 4 == 0 and Y, bias, mask 16-byte aligned: the epilogue runs on 16-byte pieces
};

static __device__ __forceinline__ f32x4 ld_guard4(const float* row, int j, int J, bool rowok, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!rowok) return v;
    if (vec && j + 3 < J) return ld4(row + j);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (j + r < J) v[r] = row[j + r];
    return v;
}

static __device__ __forceinline__ float act_apply(float v, int act) {
    switch (act) {
        case 1: return fmaxf(v, 0.f);
        case 2: return tanhf(v);
        case 3: return 1.0f / (1.0f + expf(-v));
        default: return v;
    }
}

// WG = 4 waves; a wave owns CT column tiles x RT output tiles, and ``ksplit`` waves of the WG share one such block, splitting
// the reduction range (partials combined through LDS).  Operands of U k-steps are fetched back to back before their MFMAs, so
// one memory round trip is paid per 16*U reduction indices.  Two instantiations:
//   <1,1,8>  latency mode (few columns: 32 .. 1024): 16 x 16 block per WG, 4-way K split -> one or two round trips per launch;
//   <4,4,2>  throughput mode (NBA / long batches): 64 columns x 64 outputs per wave, weight fragments reused over 4 column tiles.
template <int RT, int CT, int U>
static __device__ __forceinline__ void tlinear_body(const TLin& a, int ksplit, int bx, int by, f32x4 (*part)[RT * CT][64]) {
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4, wave = threadIdx.x >> 6;
    const int blocks_per_wg = 4 / ksplit;
    const int oblock = by * blocks_per_wg + wave / ksplit, ksub = wave % ksplit;
    const int it0 = oblock * RT;
    const bool active = it0 * 16 < a.I;
    int col[CT];
    bool colok[CT];
    const float* xrow[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        col[t] = (bx * CT + t) * 16 + c;
        colok[t] = col[t] < a.cols;
        xrow[t] = a.X + (long)((colok[t] ? col[t] : 0) / a.xdiv) * a.ldx;
    }
    f32x4 acc[RT][CT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int t = 0; t < CT; ++t) acc[i][t] = splat4(0.f);
    if (active) {
        for (int j0 = ksub * 16 * U; j0 < a.J; j0 += 16 * U * ksplit) {
            f32x4 b[U][CT], w[U][RT];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + 16 * u + 4 * q;
#pragma unroll
                for (int t = 0; t < CT; ++t) b[u][t] = ld_guard4(xrow[t], j, a.J, colok[t], a.xvec);
#pragma unroll
                for (int i = 0; i < RT; ++i) {
                    const int row = (it0 + i) * 16 + c;  // A-operand row held by this lane
                    f32x4 wv = {0.f, 0.f, 0.f, 0.f};
                    if (row < a.I) {
                        if (!a.trans) {
                            wv = ld_guard4(a.W + (long)row * a.ldw, j, a.J, true, a.wvec);
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (j + r < a.J) wv[r] = a.W[(long)(j + r) * a.ldw + row];
                        }
                    }
                    w[u][i] = wv;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int i = 0; i < RT; ++i)
#pragma unroll
                    for (int t = 0; t < CT; ++t) acc[i][t] = mfma_k16(acc[i][t], w[u][i], b[u][t]);
        }
    }
    if (ksplit > 1) {
        // waves of one block are consecutive: block leader = wave - ksub; partial slot = (leader's block) * (ksplit-1) + ksub - 1
        const int slot = (wave / ksplit) * (ksplit - 1) + ksub - 1;
        if (ksub > 0)
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int t = 0; t < CT; ++t) part[slot][i * CT + t][lane] = acc[i][t];
        __syncthreads();
        if (ksub == 0)
            for (int k = 1; k < ksplit; ++k)
#pragma unroll
                for (int i = 0; i < RT; ++i)
#pragma unroll
                    for (int t = 0; t < CT; ++t) acc[i][t] += part[(wave / ksplit) * (ksplit - 1) + k - 1][i * CT + t][lane];
    }
    if (!active || ksub != 0) return;
    if (a.evec) {
        // every operand of the epilogue in 16-byte pieces, all requested before the first is used (element by element, each load under its
        // own bounds check is followed by its own wait: 4-12 dependent L2 round trips in a kernel that lasts 5-9 us at scene sizes)
        f32x4 bv[RT], yv[RT][CT], mv[RT][CT];
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const int o = (it0 + i) * 16 + 4 * q, oc = o < a.I ? o : 0;   // (I % 4 == 0: a piece is inside or outside as a whole)
            if (a.bias) bv[i] = ld4(a.bias + oc);
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const long cc = colok[t] ? col[t] : 0;
                if (a.accumulate) yv[i][t] = ld4(a.asrc + (cc / a.adiv) * a.ldas + oc);
                if (a.mask) mv[i][t] = ld4(a.mask + cc * a.ldm + oc);
            }
        }
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const int o = (it0 + i) * 16 + 4 * q;
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                f32x4 v = acc[i][t];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float x = v[r];
                    if (a.bias) x += bv[i][r];
                    if (a.accumulate) x += yv[i][t][r];
                    x = act_apply(x, a.act);
                    if (a.mask && !(mv[i][t][r] > 0.f)) x = 0.f;
                    v[r] = x;
                }
                if (colok[t] && o < a.I) st4(a.Y + (long)col[t] * a.ldy + o, v);
            }
        }
        return;
    }
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        if (!colok[t]) continue;
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const int o = (it0 + i) * 16 + 4 * q;
            if (o >= a.I) continue;
            float* yp = a.Y + (long)col[t] * a.ldy + o;
            f32x4 v = acc[i][t];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (o + r >= a.I) continue;
                float x = v[r];
                if (a.bias) x += a.bias[o + r];
                if (a.accumulate) x += a.asrc[(long)(col[t] / a.adiv) * a.ldas + o + r];
                x = act_apply(x, a.act);
                if (a.mask && !(a.mask[(long)col[t] * a.ldm + o + r] > 0.f)) x = 0.f;
                v[r] = x;
            }
            if (a.yvec && o + 3 < a.I) st4(yp, v);
            else
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (o + r < a.I) yp[r] = v[r];
        }
    }
}

template <int RT, int CT, int U>
__global__ __launch_bounds__(256) void tlinear_kernel(TLin a, int ksplit) {
    __shared__ f32x4 part[3][RT * CT][64];
    tlinear_body<RT, CT, U>(a, ksplit, blockIdx.x, blockIdx.y, part);
}

// ---------------------------------------------------------------------------------------------------
// tgemm (round 4): the three products of nn.Linear's training step at BATCH sizes (more than 2048 columns: NBA batches, scene batches)
//     forward          Y [c][i]  = act(sum_j X[c / xdiv][j] W[i][j] + b[i])         (train.py:83 -> model/STTODE.py:553-568)
//     input gradient   dX[c][k]  = mask(sum_n dY[c][n] W[n][k] (+ dX[c][k]))
//     weight gradient  dW[n][k] += sum_c dY[c][n] X[c / xdiv][k],   db[n] += sum_c dY[c][n]
// as ONE LDS-tiled kernel  C[m][n] (+)= sum_k A(m, k) B(n, k).  The generic kernels above read every MFMA operand straight from global
// memory with per-lane 16-byte (or, for the transposed operands, four strided 4-byte) loads and no look-ahead: 0.35-0.39 of the fp32 MFMA
// peak, bound by operand-load latency (profiles/r03).  Here a workgroup owns a 64 x 64 tile of C; per 32-deep k tile all 256 threads
// fetch the two 64 x 32 operand panels with coalesced 16-byte loads -- along k where k is the contiguous index, along the row index and
// transposed on the way into LDS where it is not -- one k tile AHEAD of the MFMAs (registers -> the other LDS buffer), and every wave
// computes a 32 x 32 block with v_mfma_f32_32x32x2_f32 from 16-byte LDS reads (rows padded to 36 words: conflict-free).
// MFMA step 4g + r consumes the k pair (8g + r, 8g + 4 + r): both operands are read as f32x4 at k = 8g + 4h + (0..3) by lane half h.
// ---------------------------------------------------------------------------------------------------
struct TG {
    const float* A; const float* B; float* C;
    long lda, ldb, ldc;
    int M, N, Kt;            // C is M x N, the reduction runs over Kt
    int adiv, bkdiv;         // row of A = m / adiv (A not transposed: tlinear's broadcast rows); reduction index of B = k / bkdiv (twgrad's X rows)
    int ones_row;            // twgrad: B(n == ones_row, .) = 1 -- the bias gradient rides as one more column of dW; -1: none
    int avec, bvec, cvec;    // operand / result rows 16-byte aligned
    int evec;                // mode 0: N % 4 == 0 and C, bias, mask 16-byte aligned -- the epilogue runs on 16-byte pieces
    int fast;                // operands fit tg_fetch_fast (tg_fast below)
    long long* dbg;          // diagnostic (sttode_tgemm_debug_buffer): [workgroup][4] stamps of the 100 MHz clock -- start, first tile in LDS, reduction done, end
    const float* bias; const float* mask; long ldm; int act, accumulate;   // mode 0 (tlinear) epilogue
    const float* asrc; long ldas; int acdiv;                               // `accumulate` adds row (m / acdiv) of asrc (TLin::asrc)
    float* db; float* scratch; int S, kchunk, mode;                        // mode 1 (twgrad): split s = blockIdx.z reduces k in [s kchunk, (s + 1) kchunk)
};

typedef float tg_f32x16 __attribute__((ext_vector_type(16)));

// one 64 x 32 operand panel: 2 x f32x4 per thread.  T = false: memory is [row][k] (k contiguous): thread -> (row, 4 k); T = true: memory is
// [k][row] (row contiguous): thread -> (k, 4 rows), transposed when stored to LDS.
template <bool T>
static __device__ __forceinline__ void tg_fetch(f32x4 (&v)[2], const float* __restrict__ src, long ld, int row0, int rows, int rdiv, int k0, int kend,
                                                int kdiv, int ones_row, bool vec) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int idx = (int)threadIdx.x + 256 * p;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (!T) {
            const int row = row0 + (idx >> 3), k = k0 + (idx & 7) * 4;
            if (row < rows && k < kend) {
                const float* q = src + (long)(row / rdiv) * ld + k;
                if (vec && k + 3 < kend) x = ld4(q);
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (k + e < kend) x[e] = q[e];
                }
            }
        } else {
            const int k = k0 + (idx >> 4), row = row0 + (idx & 15) * 4;
            if (k < kend && row < rows + (ones_row >= 0 ? 1 : 0)) {
                const float* q = src + (long)(k / kdiv) * ld + row;
                if (vec && row + 3 < rows) x = ld4(q);
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (row + e < rows) x[e] = q[e];
                        else if (row + e == ones_row) x[e] = 1.0f;
                }
            }
        }
        v[p] = x;
    }
}
// LDS panel of one operand (2304 floats).  T = false: [64 rows][36] (k contiguous, rows padded to 36 words: 16-byte stores and 16-byte
// fragment reads, conflict-free).  T = true: [32 k][68] (rows contiguous: the transposed source's 16-byte pieces are stored as they are;
// the fragment is read as four 4-byte words, lanes on consecutive rows -- transposing on the way IN, four scalar stores at a stride of
// 36 words, is an 8-way bank conflict: measured 36 us per weight gradient against 34.5 us for the generic kernel).
#define TG_PANEL 2304
template <bool T>
static __device__ __forceinline__ void tg_store(const f32x4 (&v)[2], float* S) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int idx = (int)threadIdx.x + 256 * p;
        if (!T) *reinterpret_cast<f32x4*>(S + (idx >> 3) * 36 + (idx & 7) * 4) = v[p];
        else *reinterpret_cast<f32x4*>(S + (idx >> 4) * 68 + (idx & 15) * 4) = v[p];
    }
}
// the fragment of MFMA steps 4q .. 4q + 3 for row `row` (0..63) of the panel: k = 8q + 4h + (0..3)
template <bool T>
static __device__ __forceinline__ f32x4 tg_frag(const float* S, int row, int q, int h) {
    if (!T) return *reinterpret_cast<const f32x4*>(S + row * 36 + 8 * q + 4 * h);
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = S[(8 * q + 4 * h + e) * 68 + row];
    return r;
}

// Branch-free form of tg_fetch for the shapes the training step is made of (g.fast: 16-byte aligned operands, no broadcast rows, the
// contiguous index a multiple of 4): addresses are clamped into the operand instead of tested, pieces beyond [.., kend) are zeroed by a
// select.  Without branches the compiler counts outstanding loads exactly, and a tile can be requested TWO tiles ahead: a 64 x 64 tile
// needs 16 KB per 32-deep step for 262 kFLOP -- at the MFMA rate that is 38 GB/s per CU, 9.6 TB/s chip-wide out of L2 -- and with one
// tile in flight per workgroup the step lasted one loaded L2 round trip instead (measured 30 us for a product with 12 us of MFMA).
template <bool T>
static __device__ __forceinline__ void tg_fetch_fast(f32x4 (&v)[2], const float* __restrict__ src, long ld, int row0, int rows, int k0, int kend) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int idx = (int)threadIdx.x + 256 * p;
        if (!T) {
            const int row = row0 + (idx >> 3), k = k0 + (idx & 7) * 4;
            v[p] = ld4(src + (long)(row < rows ? row : rows - 1) * ld + (k < kend ? k : kend - 4));
        } else {
            const int k = k0 + (idx >> 4), row = row0 + (idx & 15) * 4;
            v[p] = ld4(src + (long)(k < kend ? k : kend - 1) * ld + (row + 3 < rows ? row : rows - 4));
        }
    }
}
// ... and what the bounds tests would have done, applied when the tile goes to LDS (not at the request: the selects would wait for the data)
template <bool T>
static __device__ __forceinline__ void tg_store_fast(f32x4 (&v)[2], float* S, int row0, int k0, int kend, int ones_row) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int idx = (int)threadIdx.x + 256 * p;
        f32x4 x = v[p];
        if (!T) {
            if (!(k0 + (idx & 7) * 4 < kend)) x = splat4(0.f);
            *reinterpret_cast<f32x4*>(S + (idx >> 3) * 36 + (idx & 7) * 4) = x;
        } else {
            const int row = row0 + (idx & 15) * 4;
            if (ones_row >= 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (row + e == ones_row) x[e] = 1.0f;
            }
            if (!(k0 + (idx >> 4) < kend)) x = splat4(0.f);
            *reinterpret_cast<f32x4*>(S + (idx >> 4) * 68 + (idx & 15) * 4) = x;
        }
    }
}

template <bool AT, bool BT>
static __device__ __forceinline__ void tg_mma_tile(tg_f32x16& acc, const float* Sa, const float* Sb, int mt, int nt, int c, int h) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 b = tg_frag<AT>(Sa, mt * 32 + c, q, h);     // MFMA columns = m
        const f32x4 a = tg_frag<BT>(Sb, nt * 32 + c, q, h);     // MFMA rows = n
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r], b[r], acc, 0, 0, 0);
    }
}

static __device__ __forceinline__ void tg_epilogue(const TG& g, const tg_f32x16& acc, int m0, int n0, int mt, int nt, int c, int h, int bz);
// one 64 x 64 tile of C (tile indices bx, by; bz: the split of the reduction in mode 1) by the calling workgroup
template <bool AT, bool BT>
static __device__ __forceinline__ void tgemm_body(const TG& g, int bx, int by, int bz, float (*As)[TG_PANEL], float (*Bs)[TG_PANEL]) {
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
    const int m0 = bx * 64, n0 = by * 64;
    const int kbeg = g.mode == 1 ? bz * g.kchunk : 0;
    const int kend = g.mode == 1 ? (kbeg + g.kchunk < g.Kt ? kbeg + g.kchunk : g.Kt) : g.Kt;
    const int mt = wave & 1, nt = wave >> 1;
    tg_f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    f32x4 va[2], vb[2];
    const int brows = g.N - (g.ones_row >= 0 ? 1 : 0);
    const int wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (g.dbg && threadIdx.x == 0) g.dbg[4 * wg] = __builtin_amdgcn_s_memrealtime();
    if (g.fast && kbeg < kend) {
        // two tiles ahead: register set 0 / 1 holds tile t / t + 1 on its way to LDS buffer 0 / 1 (requests beyond the last tile read one
        // clamped piece and give zeros); lds_barrier(): the workgroup barrier WITHOUT the vmcnt(0) of __syncthreads(), which would drain
        // the requests of the tile after next at every step
        f32x4 ua[2], ub[2];
        const int P = (kend - kbeg + 31) / 32;
        tg_fetch_fast<AT>(va, g.A, g.lda, m0, g.M, kbeg, kend);
        tg_fetch_fast<BT>(vb, g.B, g.ldb, n0, brows, kbeg, kend);
        tg_fetch_fast<AT>(ua, g.A, g.lda, m0, g.M, kbeg + 32, kend);
        tg_fetch_fast<BT>(ub, g.B, g.ldb, n0, brows, kbeg + 32, kend);
        __builtin_amdgcn_sched_barrier(0);
        tg_store_fast<AT>(va, As[0], m0, kbeg, kend, -1);
        tg_store_fast<BT>(vb, Bs[0], n0, kbeg, kend, g.ones_row);
        lds_barrier();
        if (g.dbg && threadIdx.x == 0) g.dbg[4 * wg + 1] = __builtin_amdgcn_s_memrealtime();
        int t = 0;
        for (; t + 2 <= P; t += 2) {
            const int k1 = kbeg + 32 * (t + 1);
            tg_fetch_fast<AT>(va, g.A, g.lda, m0, g.M, k1 + 32, kend);
            tg_fetch_fast<BT>(vb, g.B, g.ldb, n0, brows, k1 + 32, kend);
            __builtin_amdgcn_sched_barrier(0);               // (the scheduler otherwise sinks the requests to their first use, behind the MFMAs)
            tg_mma_tile<AT, BT>(acc, As[0], Bs[0], mt, nt, c, h);
            __builtin_amdgcn_sched_barrier(0);
            tg_store_fast<AT>(ua, As[1], m0, k1, kend, -1);
            tg_store_fast<BT>(ub, Bs[1], n0, k1, kend, g.ones_row);
            lds_barrier();
            tg_fetch_fast<AT>(ua, g.A, g.lda, m0, g.M, k1 + 64, kend);
            tg_fetch_fast<BT>(ub, g.B, g.ldb, n0, brows, k1 + 64, kend);
            __builtin_amdgcn_sched_barrier(0);
            tg_mma_tile<AT, BT>(acc, As[1], Bs[1], mt, nt, c, h);
            __builtin_amdgcn_sched_barrier(0);
            tg_store_fast<AT>(va, As[0], m0, k1 + 32, kend, -1);
            tg_store_fast<BT>(vb, Bs[0], n0, k1 + 32, kend, g.ones_row);
            lds_barrier();
        }
        if (t < P) tg_mma_tile<AT, BT>(acc, As[0], Bs[0], mt, nt, c, h);
    } else {
    tg_fetch<AT>(va, g.A, g.lda, m0, g.M, g.adiv, kbeg, kend, 1, -1, g.avec);
    tg_fetch<BT>(vb, g.B, g.ldb, n0, brows, 1, kbeg, kend, g.bkdiv, g.ones_row, g.bvec);
    tg_store<AT>(va, As[0]);
    tg_store<BT>(vb, Bs[0]);
    __syncthreads();
    int buf = 0;
    for (int k0 = kbeg; k0 < kend; k0 += 32) {
        const bool more = k0 + 32 < kend;
        if (more) {   // the next k tile travels while this one is multiplied
            tg_fetch<AT>(va, g.A, g.lda, m0, g.M, g.adiv, k0 + 32, kend, 1, -1, g.avec);
            tg_fetch<BT>(vb, g.B, g.ldb, n0, brows, 1, k0 + 32, kend, g.bkdiv, g.ones_row, g.bvec);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 b = tg_frag<AT>(As[buf], mt * 32 + c, q, h);     // MFMA columns = m
            const f32x4 a = tg_frag<BT>(Bs[buf], nt * 32 + c, q, h);     // MFMA rows = n
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r], b[r], acc, 0, 0, 0);
        }
        if (more) {
            tg_store<AT>(va, As[buf ^ 1]);
            tg_store<BT>(vb, Bs[buf ^ 1]);
        }
        __syncthreads();
        buf ^= 1;
    }
    }
    if (g.dbg && threadIdx.x == 0) g.dbg[4 * wg + 2] = __builtin_amdgcn_s_memrealtime();
    tg_epilogue(g, acc, m0, n0, mt, nt, c, h, bz);
    if (g.dbg) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0) g.dbg[4 * wg + 3] = __builtin_amdgcn_s_memrealtime();
    }
}
static __device__ __forceinline__ void tg_epilogue(const TG& g, const tg_f32x16& acc, int m0, int n0, int mt, int nt, int c, int h, int bz) {
    // lane (c, h): m = m0 + 32 mt + c; register 4a + b <-> n = n0 + 32 nt + 8a + 4h + b
    const int m = m0 + mt * 32 + c;
    if (m >= g.M) return;
    if (g.mode == 1 && g.S > 1) {
        // split reduction: the partial tile goes to scratch [split][M][N]; the splits are added in order by a reduction launch (deterministic).
        // (Combining inside the launch -- last workgroup of a tile, ticket counter -- was built and measured: the agent-scope release every
        // workgroup needs before its ticket writes the whole L2 back on this part, 183 us per weight gradient against 36 us + 10 us.)
        float* part = g.scratch + ((long)bz * g.M + m) * g.N;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int n = n0 + nt * 32 + 8 * a + 4 * h;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (n + e < g.N) part[n + e] = acc[4 * a + e];
        }
        return;
    }
    if (g.mode == 0 && g.evec) {
        // every operand of the epilogue in 16-byte pieces, all requested before the first is used (element by element under its bounds
        // check each load is followed by its own wait: 16-48 dependent L2 round trips per lane, 5-10 us of a 25-us product)
        f32x4 bv[4], yv[4], mv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int n = n0 + nt * 32 + 8 * a + 4 * h;
            const int nc = n < g.N ? n : 0;                   // (N % 4 == 0: a piece is inside or outside as a whole)
            if (g.bias) bv[a] = ld4(g.bias + nc);
            if (g.accumulate) yv[a] = ld4(g.asrc + (long)(m / g.acdiv) * g.ldas + nc);
            if (g.mask) mv[a] = ld4(g.mask + (long)m * g.ldm + nc);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int n = n0 + nt * 32 + 8 * a + 4 * h;
            f32x4 v = {acc[4 * a], acc[4 * a + 1], acc[4 * a + 2], acc[4 * a + 3]};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float x = v[e];
                if (g.bias) x += bv[a][e];
                if (g.accumulate) x += yv[a][e];
                x = act_apply(x, g.act);
                if (g.mask && !(mv[a][e] > 0.f)) x = 0.f;
                v[e] = x;
            }
            if (n < g.N) st4(g.C + (long)m * g.ldc + n, v);
        }
        return;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int n = n0 + nt * 32 + 8 * a + 4 * h;
        if (n >= g.N) continue;
        f32x4 v = {acc[4 * a], acc[4 * a + 1], acc[4 * a + 2], acc[4 * a + 3]};
        if (g.mode == 0) {
            float* yp = g.C + (long)m * g.ldc + n;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (n + e >= g.N) continue;
                float x = v[e];
                if (g.bias) x += g.bias[n + e];
                if (g.accumulate) x += g.asrc[(long)(m / g.acdiv) * g.ldas + n + e];
                x = act_apply(x, g.act);
                if (g.mask && !(g.mask[(long)m * g.ldm + n + e] > 0.f)) x = 0.f;
                v[e] = x;
            }
            if (g.cvec && n + 3 < g.N) st4(yp, v);
            else
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (n + e < g.N) yp[e] = v[e];
        } else {
            const int K = g.N - 1;   // the last column of C is the bias gradient
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (n + e >= g.N) continue;
                if (n + e < K) g.C[(long)m * g.ldc + n + e] += v[e];        // (S == 1; the split case returned above)
                else if (g.db) g.db[m] += v[e];
            }
        }
    }
}

template <bool AT, bool BT>
__global__ __launch_bounds__(256) void tgemm_kernel(TG g) {
    __shared__ __attribute__((aligned(16))) float As[2][TG_PANEL];
    __shared__ __attribute__((aligned(16))) float Bs[2][TG_PANEL];
    tgemm_body<AT, BT>(g, blockIdx.x, blockIdx.y, blockIdx.z, As, Bs);
}

// One launch for a layer's backward at batch sizes: blocks [0, nw) are the tiles x splits of the weight gradient dW = dY^T [X | 1],
// the remaining blocks the tiles of the input gradient dX = dY W -- two products that share nothing but dY and have the chip to themselves
// for 25-30 us each when launched one after the other (profiles/r04/train_shapes_before.txt: 0.31 of peak for the pair + its reduction).
__global__ __launch_bounds__(256) void tgemm_bwd_kernel(TG gw, int gxw, int gyw, int nw, TG gx, int gxx) {
    __shared__ __attribute__((aligned(16))) float As[2][TG_PANEL];
    __shared__ __attribute__((aligned(16))) float Bs[2][TG_PANEL];
    int id = blockIdx.x;
    if (id < nw) tgemm_body<true, true>(gw, id % gxw, (id / gxw) % gyw, id / (gxw * gyw), As, Bs);
    else {
        id -= nw;
        tgemm_body<false, true>(gx, id % gxx, id / gxx, 0, As, Bs);
    }
}

// Several independent products in ONE launch (sttode_tgemm_group): a 2-GFLOP product is one round of ~930 workgroups on 1024 slots and
// pays ~7 us of start skew, first tile and store burst around 16 us of MFMA (profiles/r04/tgemm_workgroup_trace.txt); with the decoder's
// decoder_x / decoder_y layers (same input, separate weights) or a layer's dX / dW side by side, a later product's workgroups start as an
// earlier one's finish.  Problem p owns blocks [blk0[p], blk0[p + 1]); kind: 0 forward, 1 input gradient, 2 weight gradient.
#define TG_MULTI_MAX 4
struct TGMulti { TG g[TG_MULTI_MAX]; int blk0[TG_MULTI_MAX + 1]; int gx[TG_MULTI_MAX], gy[TG_MULTI_MAX], kind[TG_MULTI_MAX]; int n; };
__global__ __launch_bounds__(256) void tgemm_multi_kernel(TGMulti M) {
    __shared__ __attribute__((aligned(16))) float As[2][TG_PANEL];
    __shared__ __attribute__((aligned(16))) float Bs[2][TG_PANEL];
    int p = 0;
    while (p + 1 < M.n && (int)blockIdx.x >= M.blk0[p + 1]) ++p;
    p = __builtin_amdgcn_readfirstlane(p);
    // the problem's descriptor out of the kernel-argument segment (uniform index: scalar loads; indexing the by-value struct would park
    // all four descriptors in registers first)
    TG g;
    {
        const __attribute__((address_space(4))) int* src = (const __attribute__((address_space(4))) int*)(
            (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TGMulti, g) + (size_t)p * sizeof(TG));
        int* dst = reinterpret_cast<int*>(&g);
#pragma unroll
        for (unsigned i = 0; i < sizeof(TG) / 4; ++i) dst[i] = src[i];
    }
    const int id = (int)blockIdx.x - M.blk0[p], gx = M.gx[p], gy = M.gy[p], kind = M.kind[p];
    const int bx = id % gx, by = (id / gx) % gy, bz = id / (gx * gy);
    if (kind == 0) tgemm_body<false, false>(g, bx, by, bz, As, Bs);
    else if (kind == 1) tgemm_body<false, true>(g, bx, by, bz, As, Bs);
    else tgemm_body<true, true>(g, bx, by, bz, As, Bs);
}

// Deferred reductions of split weight gradients: up to TG_RED_MAX of them are added into their dW / db by ONE launch (twenty 10-us launches
// per NBA-size step otherwise).  Item i owns blocks [blk0[i], blk0[i + 1]).
#define TG_RED_MAX 16
struct TGRedItem { const float* part; float* dW; float* db; long ldw; long per; int K1, S, blk0; };
struct TGRed { TGRedItem it[TG_RED_MAX]; int n; };
__global__ __launch_bounds__(256) void tgemm_reduce_kernel(TGRed r) {
    int i = 0;
    while (i + 1 < r.n && (int)blockIdx.x >= r.it[i + 1].blk0) ++i;
    const TGRedItem& t = r.it[i];
    const long e = (long)(blockIdx.x - t.blk0) * 256 + threadIdx.x;
    if (e >= t.per) return;
    const int n = (int)(e / t.K1), k = (int)(e % t.K1);
    float tot = 0.f;
    for (int s = 0; s < t.S; ++s) tot += t.part[(long)s * t.per + e];
    if (k < t.K1 - 1) t.dW[(long)n * t.ldw + k] += tot;
    else if (t.db) t.db[n] += tot;
}

// ---------------------------------------------------------------------------------------------------
// twgrad: WG = 4 waves own a 32 x 32 block of [dW | db] for one column split; waves interleave 16-column chunks
// ---------------------------------------------------------------------------------------------------
struct TWg {
    const float* dY; const float* X; float* dW; float* db; float* scratch;
    long ldy, ldx, ldw;
    int cols, N, K, xdiv, S, chunks_per_split;   // S: 1 from every caller but the one named at sttode_twgrad's reduction launch
};

static __device__ __forceinline__ void twgrad_body(const TWg& a, int bx, int by, int bz, float (*red)[32][33]) {
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4, wave = threadIdx.x >> 6;
    const int n0 = bx * 32, k0 = by * 32, s = bz;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = splat4(0.f);
    const int ch0 = s * a.chunks_per_split, ch1 = min(ch0 + a.chunks_per_split, (a.cols + 15) / 16);
    for (int ch = ch0 + wave; ch < ch1; ch += 4) {
        f32x4 av[2], bv[2];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int cc = ch * 16 + 4 * q + r;
            const bool ok = cc < a.cols;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int n = n0 + 16 * i + c;
                av[i][r] = (ok && n < a.N) ? a.dY[(long)cc * a.ldy + n] : 0.f;
                const int k = k0 + 16 * i + c;
                bv[i][r] = !ok ? 0.f : (k < a.K ? a.X[(long)(cc / a.xdiv) * a.ldx + k] : (k == a.K ? 1.0f : 0.f));
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = mfma_k16(acc[i][j], av[i], bv[j]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][16 * i + 4 * q + r][16 * j + c] = acc[i][j][r];
    __syncthreads();
    for (int e = threadIdx.x; e < 32 * 32; e += 256) {
        const int rn = e >> 5, rk = e & 31, n = n0 + rn, k = k0 + rk;
        if (n >= a.N || k > a.K) continue;
        const float tot = ((red[0][rn][rk] + red[1][rn][rk]) + red[2][rn][rk]) + red[3][rn][rk];
        if (a.S == 1) {
            if (k < a.K) a.dW[(long)n * a.ldw + k] += tot;
            else if (a.db) a.db[n] += tot;
        } else {
            a.scratch[((long)s * a.N + n) * (a.K + 1) + k] = tot;
        }
    }
}

__global__ __launch_bounds__(256) void twgrad_kernel(TWg a) {
    __shared__ float red[4][32][33];
    twgrad_body(a, blockIdx.x, blockIdx.y, blockIdx.z, red);
}

// One launch for a layer's backward at training-scene sizes: blocks [0, nA) compute the input gradient (tlinear latency mode),
// the remaining blocks the weight / bias gradient.  The two halves are independent (dX must not alias dY or X).
__global__ __launch_bounds__(256) void tbwd_kernel(TLin a, int ksplit, int gxA, int nA, TWg w, int gxW, int gyW) {
    __shared__ __attribute__((aligned(16))) char sm[4 * 32 * 33 * 4];
    int id = blockIdx.x;
    if (id < nA) {
        tlinear_body<1, 1, 8>(a, ksplit, id % gxA, id / gxA, reinterpret_cast<f32x4(*)[1][64]>(sm));
    } else {
        id -= nA;
        twgrad_body(w, id % gxW, (id / gxW) % gyW, id / (gxW * gyW), reinterpret_cast<float(*)[32][33]>(sm));
    }
}

__global__ void twgrad_reduce_kernel(TWg a) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = (long)a.N * (a.K + 1);
    if (e >= per) return;
    const int n = (int)(e / (a.K + 1)), k = (int)(e % (a.K + 1));
    float tot = 0.f;
    for (int s = 0; s < a.S; ++s) tot += a.scratch[(long)s * per + e];
    if (k < a.K) a.dW[(long)n * a.ldw + k] += tot;
    else if (a.db) a.db[n] += tot;
}

// Scene sizes (cols <= 1024), grouped (sttode_tgemm_group): up to four independent layers -- forward (kind 0) or a whole backward (kind 1:
// input-gradient blocks, then weight-gradient blocks, as tbwd_kernel) -- in ONE launch.  A one-scene training step is bound by the NUMBER
// of launches (~5 us per dependent graph node whatever it does): decoder_x / decoder_y of a block and the two encoder trunks walk through
// the same layers with different weights.
#define TS_MULTI_MAX 4
struct TSProb { TLin a; TWg w; int ksplit, gxA, nA, gxW, gyW, kind; };
struct TSMulti { TSProb p[TS_MULTI_MAX]; int blk0[TS_MULTI_MAX + 1]; int n; };
__global__ __launch_bounds__(256) void tsmall_multi_kernel(TSMulti M) {
    __shared__ __attribute__((aligned(16))) char sm[4 * 32 * 33 * 4];
    int p = 0;
    while (p + 1 < M.n && (int)blockIdx.x >= M.blk0[p + 1]) ++p;
    p = __builtin_amdgcn_readfirstlane(p);
    TSProb P;   // the problem's descriptor out of the kernel-argument segment (uniform index: scalar loads)
    {
        const __attribute__((address_space(4))) int* src = (const __attribute__((address_space(4))) int*)(
            (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TSMulti, p) + (size_t)p * sizeof(TSProb));
        int* dst = reinterpret_cast<int*>(&P);
#pragma unroll
        for (unsigned i = 0; i < sizeof(TSProb) / 4; ++i) dst[i] = src[i];
    }
    int id = (int)blockIdx.x - M.blk0[p];
    if (P.kind == 0 || id < P.nA) tlinear_body<1, 1, 8>(P.a, P.ksplit, id % P.gxA, id / P.gxA, reinterpret_cast<f32x4(*)[1][64]>(sm));
    else {
        id -= P.nA;
        twgrad_body(P.w, id % P.gxW, (id / P.gxW) % P.gyW, id / (P.gxW * P.gyW), reinterpret_cast<float(*)[32][33]>(sm));
    }
}

#ifndef TLIN_MEDIUM_BELOW
#define TLIN_MEDIUM_BELOW 4096   // throughput-mode wave count below which the 32 x 32 tiling is used instead
#endif

// columns above which the LDS-tiled kernel takes over from the generic ones (measured at 1024: the one-scene step the same 1.04-1.08 ms,
// and the NBA 16 x 11 gradient yardstick fails -- profiles/r04/tgemm_min_cols_ab.txt)
// Round 5: the BACKWARD products (input gradient, weight gradient) switch at 600 columns (TGEMM_MIN_COLS_BWD; training.py allocates its
// reduction scratch by the same number).  With the decoder's
// backward over the live columns only, an NBA-size step's backward products have 2 n = 704 columns -- below 2048, on the generic kernels:
// 1.155 -> 1.086 ms per step with the LDS-tiled kernel (profiles/r05/train_tgemm_min_cols_ab.txt, measured with both thresholds at 600;
// the forward products keep 2048: at 600 the forward of a 32-agent scene (672 columns) changes its summation order and three gradient
// yardsticks on the known ill-conditioned rows move from 0.8 to 1.05-1.8 of their bounds, for no gain at one scene per step).
static constexpr int TGEMM_MIN_COLS = 2048, TGEMM_MIN_COLS_BWD = 600;
static inline int aligned16(const void* p, long ld) { return (((size_t)p) % 16 == 0) && (ld % 4 == 0); }

// ---- the descriptors: one function fills each, starting from zeros (the kernels declare them without an initial value and copy them
// whole out of the kernel arguments, so the structs themselves stay plain: no default member initialisers) ---------------------------------
// A linear product as its caller states it: Y[c] = epi(Wop X[c / xdiv]), `accumulate` adding row (c / adiv) of asrc.
// evec: a layer's input gradient (sttode_tlinear_bwd) passes asrc = Y = dX and ldas = ldy, so its accumulate term repeats the yvec term
// and its absent bias drops out: the backward case needs no expression of its own.
static TLin tlin_fill(const float* X, long ldx, int xdiv, const float* W, long ldw, int trans, const float* bias, const float* mask, long ldm,
                      float* Y, long ldy, int cols, int J, int I, int act, int accumulate, const float* asrc, long ldas, int adiv) {
    TLin a{};
    a.X = X; a.W = W; a.bias = bias; a.mask = mask; a.Y = Y;
    a.ldx = ldx; a.ldw = ldw; a.ldy = ldy; a.ldm = ldm;
    a.cols = cols; a.J = J; a.I = I; a.trans = trans; a.act = act; a.accumulate = accumulate; a.xdiv = xdiv;
    a.asrc = asrc; a.ldas = ldas; a.adiv = adiv;
    a.xvec = aligned16(X, ldx); a.wvec = aligned16(W, ldw); a.yvec = aligned16(Y, ldy);
    a.evec = I % 4 == 0 && a.yvec && (!bias || aligned16(bias, 4)) && (!mask || aligned16(mask, ldm)) && (!accumulate || aligned16(asrc, ldas));
    return a;
}
// latency mode: one 16 x 16 block per WG, reduction split over up to 4 waves (128 indices per round trip and wave)
struct TLatPlan { int ksplit, gx, gy; };
static TLatPlan tlin_latency_plan(int cols, int J, int I) {
    const int ksplit = J > 256 ? 4 : (J > 128 ? 2 : 1);
    const int blocks_per_wg = 4 / ksplit;
    return {ksplit, (cols + 15) / 16, ((I + 15) / 16 + blocks_per_wg - 1) / blocks_per_wg};
}
// tg_fetch_fast: aligned operands without broadcast rows; the contiguous index of each operand (k, or the row index of a transposed one)
// a multiple of 4 and at least 4; every split of the reduction a multiple of 4 long
static inline int tg_fast(const TG& g, bool AT, bool BT) {
    const int brows = g.N - (g.ones_row >= 0 ? 1 : 0);
    if (!g.avec || !g.bvec || g.adiv != 1 || g.bkdiv != 1 || g.Kt < 4) return 0;
    if (AT ? (g.M % 4 != 0 || g.M < 4) : g.Kt % 4 != 0) return 0;
    if (BT ? (brows % 4 != 0 || brows < 4) : g.Kt % 4 != 0) return 0;
    return 1;
}
// g_tg_dbg: a plain global, shared by every host thread: written only by this diagnostic and read once per stand-alone launch
static long long* g_tg_dbg = nullptr;
extern "C" int sttode_tgemm_debug_buffer(void* p) { g_tg_dbg = (long long*)p; return 0; }   // diagnostic: >= grid * 4 int64 (NULL: off); stand-alone launches only
// the linear product `a` (forward, or with a.trans an input gradient) on the LDS-tiled kernel: mode 0.  dbg: g_tg_dbg for a product that
// is a launch (or a group member) of its own, null for one that shares tgemm_bwd_kernel's launch
static TG tg_linear(const TLin& a, long long* dbg) {
    TG g{};
    g.A = a.X; g.lda = a.ldx; g.B = a.W; g.ldb = a.ldw; g.C = a.Y; g.ldc = a.ldy;
    g.M = a.cols; g.N = a.I; g.Kt = a.J; g.adiv = a.xdiv; g.bkdiv = 1; g.ones_row = -1; g.S = 1;
    g.avec = a.xvec; g.bvec = a.wvec; g.cvec = a.yvec; g.evec = a.evec;
    g.bias = a.bias; g.mask = a.mask; g.ldm = a.ldm; g.act = a.act; g.accumulate = a.accumulate; g.asrc = a.asrc; g.ldas = a.ldas; g.acdiv = a.adiv;
    g.fast = tg_fast(g, false, a.trans != 0); g.dbg = dbg;
    return g;
}
// the generic weight gradient: fills w and returns its grid (32 x 32 blocks of [dW | db] x column splits)
static inline dim3 twg_grid(const TWg& w) { return dim3((w.N + 31) / 32, (w.K + 1 + 31) / 32, w.S); }
static dim3 twg_fill(TWg& w, const float* dY, long ldy, const float* X, long ldx, int xdiv, float* dW, long ldw, float* db, int cols, int N, int K,
                     float* scratch, long scratch_floats) {
    w = TWg{};
    w.dY = dY; w.X = X; w.dW = dW; w.db = db; w.scratch = scratch;
    w.ldy = ldy; w.ldx = ldx; w.ldw = ldw; w.cols = cols; w.N = N; w.K = K; w.xdiv = xdiv;
    const int chunks = (cols + 15) / 16;
    const long per = (long)N * (K + 1);
    int S = chunks <= 64 ? 1 : (chunks + 31) / 32;    // >= 512 columns per split; up to 1024 columns one workgroup per tile (no reduce launch)
    if (S > 64) S = 64;
    if (!scratch || per * S > scratch_floats) S = scratch && scratch_floats >= 2 * per ? (int)(scratch_floats / per) : 1;
    if (S < 1) S = 1;
    w.S = S;
    w.chunks_per_split = (chunks + S - 1) / S;
    return twg_grid(w);
}

// ---- group mode and the deferred reductions: host-side state of the CALLING THREAD --------------------------------------------------------
// g_red, g_grp and g_ts are thread_local, and nothing else is touched between an entry point's checks and its launches: a group, and a
// bracket of deferred reductions, belong to the host thread that opened them (a training step -- its group brackets, its backward pass
// with the deferred reductions -- is issued by one thread).  Another thread's calls neither see them nor wait for them: they launch at
// once on their own stream, and no lock is taken anywhere.
//
// Split weight gradients of the LDS-tiled kernel: where the partial sums go and when they are added up.
// Default: each weight gradient is followed by its own reduction launch (partial sums in the call's scratch).  Between
// sttode_twgrad_defer(1, buf, floats) and sttode_twgrad_defer(0, ..) (the training engine brackets a backward pass with them) the partial
// sums are bump-allocated from `buf` instead -- a buffer nothing else writes -- and the reductions run as ONE launch per TG_RED_MAX
// gradients, or earlier: buf full, a destination that is already pending, another stream.  Host-side state only; inside a hipGraph capture
// the flush is captured like any other launch.
static thread_local struct { TGRed r; int blocks; long used; float* buf; long cap; void* stream; bool defer; } g_red = {{}, 0, 0, nullptr, 0, nullptr, false};

static void tg_red_flush() {
    if (g_red.r.n > 0) hipLaunchKernelGGL(tgemm_reduce_kernel, dim3((unsigned)g_red.blocks), dim3(256), 0, (hipStream_t)g_red.stream, g_red.r);
    g_red.r.n = 0; g_red.blocks = 0; g_red.used = 0;
}
// after the launch that wrote g's partial sums: queue (or run) their reduction
static void tg_wgrad_done(const TG& g, float* dW, long ldw, float* db) {
    if (g.S <= 1) return;
    const long per = (long)g.M * g.N;
    if (g_red.r.n == TG_RED_MAX) tg_red_flush();
    TGRedItem& t = g_red.r.it[g_red.r.n++];
    t.part = g.scratch; t.dW = dW; t.db = db; t.ldw = ldw; t.per = per; t.K1 = g.N; t.S = g.S; t.blk0 = g_red.blocks;
    g_red.blocks += (int)((per + 255) / 256);
    const bool in_buf = g_red.buf && g.scratch >= g_red.buf && g.scratch < g_red.buf + g_red.cap;
    if (!g_red.defer || !in_buf) tg_red_flush();
}

// ---- grouped launches (sttode_tgemm_group): batch-size products queued between group(1) and group(0) leave as ONE tgemm_multi_kernel launch ----
static thread_local struct {
    TGMulti M; int gz[TG_MULTI_MAX];
    struct { float* dW; long ldw; float* db; } post[TG_MULTI_MAX];   // weight gradients: their split sums are queued for reduction AFTER the launch
    void* stream; bool on;
} g_grp = {};
static void tg_group_launch() {
    TGMulti& M = g_grp.M;
    if (M.n == 0) return;
    hipLaunchKernelGGL(tgemm_multi_kernel, dim3((unsigned)M.blk0[M.n]), dim3(256), 0, (hipStream_t)g_grp.stream, M);
    const int n = M.n;
    M.n = 0;
    for (int i = 0; i < n; ++i)
        if (M.kind[i] == 2) tg_wgrad_done(M.g[i], g_grp.post[i].dW, g_grp.post[i].ldw, g_grp.post[i].db);
}
// the queued LDS-tiled products, then every pending reduction behind them
static void tg_flush_all() { tg_group_launch(); tg_red_flush(); }

// ---- the scene-size queue: layers of at most 1024 columns queued in an open group leave as ONE tsmall_multi_kernel launch ----
static thread_local struct { TSMulti M; void* stream; } g_ts = {};
static void ts_group_forget() { g_ts.M.n = 0; }
static void ts_group_launch() {
    if (g_ts.M.n == 0) return;
    hipLaunchKernelGGL(tsmall_multi_kernel, dim3((unsigned)g_ts.M.blk0[g_ts.M.n]), dim3(256), 0, (hipStream_t)g_ts.stream, g_ts.M);
    g_ts.M.n = 0;
}

// queue (group mode) or launch one product; kind: 0 forward, 1 input gradient, 2 weight gradient (its split sums: dW, ldw, db)
static void tg_submit(const TG& g, int kind, int gx, int gy, int gz, void* stream, float* dW = nullptr, long ldw = 0, float* db = nullptr) {
    if (g_grp.on) {
        TGMulti& M = g_grp.M;
        if (M.n == TG_MULTI_MAX || (M.n > 0 && g_grp.stream != stream)) tg_group_launch();
        const int i = M.n++;
        if (i == 0) M.blk0[0] = 0;
        M.g[i] = g; M.g[i].dbg = nullptr; M.kind[i] = kind; M.gx[i] = gx; M.gy[i] = gy; g_grp.gz[i] = gz;
        M.blk0[i + 1] = M.blk0[i] + gx * gy * gz;
        g_grp.post[i].dW = dW; g_grp.post[i].ldw = ldw; g_grp.post[i].db = db;
        g_grp.stream = stream;
        return;
    }
    const dim3 grid(gx, gy, gz);
    if (kind == 0) hipLaunchKernelGGL((tgemm_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, g);
    else if (kind == 1) hipLaunchKernelGGL((tgemm_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, g);
    else {
        hipLaunchKernelGGL((tgemm_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, g);
        tg_wgrad_done(g, dW, ldw, db);
    }
}
// queue a scene-size layer of the open group: a forward (a), a weight gradient alone (w: a layer backward without input-gradient blocks)
// or a whole layer backward (both; w unsplit: at most 1024 columns)
static void ts_submit(const TLin* a, const TWg* w, void* stream) {
    TSMulti& M = g_ts.M;
    if (M.n == TS_MULTI_MAX || (M.n > 0 && g_ts.stream != stream)) ts_group_launch();
    const int i = M.n++;
    if (i == 0) M.blk0[0] = 0;
    TSProb& P = M.p[i];
    const TLatPlan lp = a ? tlin_latency_plan(a->cols, a->J, a->I) : TLatPlan{1, 1, 0};
    const dim3 gw = w ? twg_grid(*w) : dim3(0, 0, 0);
    P.a = a ? *a : TLin{}; P.w = w ? *w : TWg{};
    P.ksplit = lp.ksplit; P.gxA = lp.gx; P.nA = lp.gx * lp.gy; P.gxW = (int)gw.x; P.gyW = (int)gw.y; P.kind = w ? 1 : 0;
    M.blk0[i + 1] = M.blk0[i] + P.nA + (int)(gw.x * gw.y * gw.z);
    g_ts.stream = stream;
}

// does a gradient into N rows (of ldw) at dW, and db, write what a gradient into `rows` rows (of ld) at lo, and db2, writes?
static inline bool tg_dest_overlap(const float* dW, long N, long ldw, const float* db, const float* lo, long rows, long ld, const float* db2) {
    return (dW < lo + rows * ld && lo < dW + N * ldw) || (db && db == db2);
}
// fills g for dW (+)= dY^T [X | 1] with the reduction over the columns split S ways (about want_blocks workgroups); false: no room for partial sums
static bool tg_wgrad_fill(TG& g, const float* dY, long ldy, const float* X, long ldx, int xdiv, float* dW, long ldw, float* db, int cols, int N,
                          int K, float* scratch, long scratch_floats, int want_blocks, void* stream) {
    const long per = (long)N * (K + 1);
    const int tiles = ((N + 63) / 64) * ((K + 1 + 63) / 64);
    int S = (want_blocks + tiles - 1) / tiles;
    if (S > 64) S = 64;
    if (S > (cols + 127) / 128) S = (cols + 127) / 128;      // >= 128 columns per split
    if (S < 1) S = 1;
    if (g_red.r.n > 0 && (g_red.stream != stream || !g_red.defer)) tg_flush_all();
    const bool defer = g_red.defer && g_red.buf && g_red.cap >= 2 * per;
    if (defer && (g_red.r.n > 0 || g_grp.M.n > 0)) {
        // one launch adds every pending gradient: none of them may share a destination, and the queued, not yet launched gradients of the
        // open group count as pending destinations too (also in front of an unsplit gradient to a pending destination: it adds into dW itself)
        bool again = g_red.r.n == TG_RED_MAX || (S > 1 && g_red.used + per * S > g_red.cap);
        for (int i = 0; i < g_red.r.n && !again; ++i) {
            const TGRedItem& t = g_red.r.it[i];
            again = tg_dest_overlap(dW, N, ldw, db, t.dW, t.per / t.K1, t.ldw, t.db);
        }
        for (int i = 0; i < g_grp.M.n && !again; ++i)
            if (g_grp.M.kind[i] == 2) again = tg_dest_overlap(dW, N, ldw, db, g_grp.post[i].dW, g_grp.M.g[i].M, g_grp.post[i].ldw, g_grp.post[i].db);
        if (again) tg_flush_all();
    }
    if (!defer && g_grp.M.n > 0) {        // without a buffer of its own every split gradient uses the call's scratch: one per launch
        for (int i = 0; i < g_grp.M.n; ++i)
            if (g_grp.M.kind[i] == 2) { tg_group_launch(); break; }
    }
    float* part = defer ? g_red.buf + g_red.used : scratch;
    const long room = defer ? g_red.cap - g_red.used : scratch_floats;
    if (S > 1 && (!part || per * S > room)) S = part ? (int)(room / per) : 1;
    if (S < 1) return false;
    g_red.stream = stream;
    g = TG{};
    g.A = dY; g.lda = ldy; g.B = X; g.ldb = ldx; g.C = dW; g.ldc = ldw;
    g.M = N; g.N = K + 1; g.Kt = cols; g.adiv = 1; g.bkdiv = xdiv; g.ones_row = K; g.acdiv = 1;
    g.avec = aligned16(dY, ldy); g.bvec = aligned16(X, ldx);
    g.db = db; g.scratch = part; g.S = S; g.mode = 1; g.fast = tg_fast(g, true, true);
    if (defer && S > 1) g_red.used += per * S;     // reserved now: a second gradient of the same group must not get the same piece
    g.kchunk = ((cols + S - 1) / S + 31) / 32 * 32;
    return true;
}

// The one place that lists a group's queues, in the order a closing group flushes them: LDS-tiled, scene-size, element-wise, trunk.
extern "C" int sttode_tgemm_group(int on) {
    if (on < 0) { g_grp.M.n = 0; ts_group_forget(); }   // error paths: forget what is queued
    tg_group_launch();
    ts_group_launch();
    g_grp.on = on > 0;
    const int rc_ew = stt_ew_group(on), rc_trunk = stt_trunk_group(on);   // (both run: no queue stays open behind another's error)
    if (rc_ew || rc_trunk) return rc_ew ? rc_ew : rc_trunk;
    STT_HIP(hipGetLastError()); return 0;
}
bool stt_tgemm_group_open() { return g_grp.on; }
extern "C" int sttode_twgrad_defer(int on, float* buf, long floats) {
    if (on < 0) { g_red.r.n = 0; g_red.blocks = 0; g_red.used = 0; }      // error paths: forget what is pending
    tg_red_flush();
    g_red.defer = on > 0 && buf && floats > 0;
    g_red.buf = g_red.defer ? buf : nullptr; g_red.cap = g_red.defer ? floats : 0;
    STT_HIP(hipGetLastError()); return 0;
}
extern "C" int sttode_twgrad_flush(void) {
    tg_red_flush();
    STT_HIP(hipGetLastError()); return 0;
}

static int tlinear_impl(const TLin& a, void* stream) {
    const int cols = a.cols, J = a.J, I = a.I, trans = a.trans;
    STT_REQUIRE(a.X && a.W && a.Y, "sttode_tlinear: null pointer");
    STT_REQUIRE(cols > 0 && J > 0 && I > 0 && a.xdiv > 0, "sttode_tlinear: cols, J, I, xdiv must be positive");
    STT_REQUIRE(a.act >= 0 && a.act <= 3, "sttode_tlinear: act must be 0 none | 1 relu | 2 tanh | 3 sigmoid");
    STT_REQUIRE(a.ldx >= J && a.ldy >= I && a.ldw >= (trans ? I : J), "sttode_tlinear: leading dimension smaller than the row length");
    if (cols > (trans ? TGEMM_MIN_COLS_BWD : TGEMM_MIN_COLS)) {   // batch sizes: the LDS-tiled kernel (trans: an input gradient)
        // (NB = 2, 64 x 128 tiles, measured SLOWER at the NBA step's shapes -- 36-38 us against 19-25 us per product: 55 KB of LDS leave two
        // workgroups per CU to hide the panel loads instead of four -- and is not instantiated)
        tg_submit(tg_linear(a, g_tg_dbg), trans ? 1 : 0, (cols + 63) / 64, (I + 63) / 64, 1, stream);
    } else if (cols <= 1024) {
        if (g_grp.on) ts_submit(&a, nullptr, stream);   // an open group: queued, leaves with the group's other scene-size layers as one launch
        else {
            const TLatPlan lp = tlin_latency_plan(cols, J, I);
            hipLaunchKernelGGL((tlinear_kernel<1, 1, 8>), dim3(lp.gx, lp.gy), dim3(256), 0, (hipStream_t)stream, a, lp.ksplit);
        }
    } else if ((long)((cols + 63) / 64) * ((I + 63) / 64) < TLIN_MEDIUM_BELOW) {
        // medium mode: 32 columns x 32 outputs per wave -- 4x the waves of the throughput tiling, for launches that would
        // otherwise leave most SIMDs empty (e.g. 7040 columns x 512 outputs = 880 throughput-mode waves on 1024 SIMDs)
        const int ksplit = (I <= 32 && J > 64) ? 4 : ((I <= 64 && J > 64) ? 2 : 1);
        const int outs_per_wg = 128 / ksplit;
        dim3 grid((cols + 31) / 32, (I + outs_per_wg - 1) / outs_per_wg);
        hipLaunchKernelGGL((tlinear_kernel<2, 2, 4>), grid, dim3(256), 0, (hipStream_t)stream, a, ksplit);
    } else {
        const int ksplit = (I <= 64 && J > 64) ? 4 : ((I <= 128 && J > 64) ? 2 : 1);
        const int outs_per_wg = 256 / ksplit;
        dim3 grid((cols + 63) / 64, (I + outs_per_wg - 1) / outs_per_wg);
        hipLaunchKernelGGL((tlinear_kernel<4, 4, 2>), grid, dim3(256), 0, (hipStream_t)stream, a, ksplit);
    }
    STT_HIP(hipGetLastError()); return 0;
}
extern "C" int sttode_tlinear(const float* X, long ldx, int xdiv, const float* W, long ldw, int trans, const float* bias,
                              const float* mask, long ldm, float* Y, long ldy, int cols, int J, int I, int act, int accumulate,
                              void* stream) {
    return tlinear_impl(tlin_fill(X, ldx, xdiv, W, ldw, trans, bias, mask, ldm, Y, ldy, cols, J, I, act, accumulate, Y, ldy, 1), stream);
}
// Y[c] = act(W X[c] + tab[c / tdiv] (+ bias)): nn.Linear whose input is cat(shared, own) with the shared part's product -- the same for tdiv
// consecutive columns -- precomputed as a table (the decoder MLPs' layer 1, model/utils.py:86-95 on cat(past_feature_rep, z, state),
// model/STTODE.py:71-75,322-328: tab = W1[:, pf] pf + b1 per AGENT, W = W1[:, z | state]; half the layer's products, as in the inference chain)
extern "C" int sttode_tlinear_tab(const float* X, long ldx, const float* W, long ldw, const float* bias, const float* tab, long ldt, int tdiv,
                                  float* Y, long ldy, int cols, int J, int I, int act, void* stream) {
    STT_REQUIRE(tab && tdiv > 0 && ldt >= I, "sttode_tlinear_tab: bad table");
    return tlinear_impl(tlin_fill(X, ldx, 1, W, ldw, 0, bias, nullptr, 0, Y, ldy, cols, J, I, act, 1, tab, ldt, tdiv), stream);
}

extern "C" int sttode_twgrad(const float* dY, long ldy, const float* X, long ldx, int xdiv, float* dW, long ldw, float* db,
                             int cols, int N, int K, float* scratch, long scratch_floats, void* stream) {
    STT_REQUIRE(dY && X && dW, "sttode_twgrad: null pointer");
    STT_REQUIRE(cols > 0 && N > 0 && K > 0 && xdiv > 0, "sttode_twgrad: cols, N, K, xdiv must be positive");
    STT_REQUIRE(ldy >= N && ldx >= K && ldw >= K, "sttode_twgrad: leading dimension smaller than the row length");
    if (cols > TGEMM_MIN_COLS_BWD) {   // batch sizes: the LDS-tiled kernel, reduction over the columns split so that the chip is full
        TG g;
        if (tg_wgrad_fill(g, dY, ldy, X, ldx, xdiv, dW, ldw, db, cols, N, K, scratch, scratch_floats, 480, stream)) {
            tg_submit(g, 2, (N + 63) / 64, (K + 1 + 63) / 64, g.S, stream, dW, ldw, db);
            STT_HIP(hipGetLastError()); return 0;
        }
    }
    TWg w;
    const dim3 grid = twg_fill(w, dY, ldy, X, ldx, xdiv, dW, ldw, db, cols, N, K, scratch, scratch_floats);
    if (g_grp.on && cols <= 1024) {   // an open group: a weight gradient alone is a layer backward without input-gradient blocks
        ts_submit(nullptr, &w, stream);
        STT_HIP(hipGetLastError()); return 0;
    }
    hipLaunchKernelGGL(twgrad_kernel, grid, dim3(256), 0, (hipStream_t)stream, w);
    // The generic kernel's own split, S > 1, is left with ONE case.  Up to 600 columns there are at most 38 chunks of 16 and one split; above,
    // this line is reached only when tg_wgrad_fill found no room for one gradient's partial sums.  Without deferral that room is the call's
    // scratch, and twg_fill's test of the same scratch gives S = 1.  With deferral it is the deferral buffer, which is out of room with
    // nothing pending or queued to flush only after sttode_tgemm_group(-1) forgot a group's split gradients (their pieces stay reserved
    // until the bracket ends or is abandoned); a gradient of more than 1024 columns issued in that state splits over the call's scratch.
    // The training engine never gets here: it follows group(-1) with sttode_twgrad_defer(-1), which frees the pieces.  Only a caller of
    // the C entry points that goes on inside the bracket does.
    if (w.S > 1) hipLaunchKernelGGL(twgrad_reduce_kernel, dim3((unsigned)(((long)N * (K + 1) + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w);
    STT_HIP(hipGetLastError()); return 0;
}

// Backward of one nn.Linear in (at most) two launches: dX = mask(dY W[:, :Kdx] (+ dX)) and dW += dY^T X, db += sum dY.
// Small column counts (the launch-bound regime) take the fused kernel; otherwise the two stand-alone entry points run.
extern "C" int sttode_tlinear_bwd(const float* dY, long ldy, const float* W, long ldw, const float* mask, long ldm, float* dX,
                                  long lddx, int Kdx, int accumulate, const float* X, long ldx, int xdiv, float* dW, long ldgw,
                                  float* db, int cols, int N, int K, float* scratch, long scratch_floats, void* stream) {
    STT_REQUIRE(dY && W && dX && X && dW, "sttode_tlinear_bwd: null pointer");
    STT_REQUIRE(cols > 0 && N > 0 && K > 0 && Kdx > 0 && Kdx <= K && xdiv > 0, "sttode_tlinear_bwd: bad sizes");
    if (xdiv == 1) {   // (broadcast rows: the two stand-alone entry points, with their own checks)
        STT_REQUIRE(ldy >= N && ldx >= K && ldgw >= K && ldw >= K && lddx >= Kdx, "sttode_tlinear_bwd: leading dimension smaller than the row length");
        const TLin a = tlin_fill(dY, ldy, 1, W, ldw, 1, nullptr, mask, ldm, dX, lddx, cols, N, Kdx, 0, accumulate, dX, lddx, 1);   // the input gradient
        if (cols > TGEMM_MIN_COLS_BWD) {   // batch sizes: both products of the layer's backward in ONE launch
            const TG gx = tg_linear(a, nullptr);
            TG gw;
            const int gxx = (cols + 63) / 64, gyx = (Kdx + 63) / 64, nx = gxx * gyx;
            if (tg_wgrad_fill(gw, dY, ldy, X, ldx, 1, dW, ldgw, db, cols, N, K, scratch, scratch_floats,
                              g_grp.on ? 400 : (nx < 680 ? 1000 - nx : 320), stream)) {
                const int gxw = (N + 63) / 64, gyw = (K + 1 + 63) / 64, nw = gxw * gyw * gw.S;
                if (g_grp.on) {   // (an open group: the two products join it as two of its problems)
                    tg_submit(gw, 2, gxw, gyw, gw.S, stream, dW, ldgw, db);
                    tg_submit(gx, 1, gxx, gyx, 1, stream);
                } else {
                    hipLaunchKernelGGL(tgemm_bwd_kernel, dim3(nw + nx), dim3(256), 0, (hipStream_t)stream, gw, gxw, gyw, nw, gx, gxx);
                    tg_wgrad_done(gw, dW, ldgw, db);
                }
                STT_HIP(hipGetLastError()); return 0;
            }
        }
        if (cols <= 1024) {   // scene sizes: input-gradient blocks, then weight-gradient blocks (one split: at most 64 chunks of 16 columns)
            TWg w;
            const dim3 gridW = twg_fill(w, dY, ldy, X, ldx, 1, dW, ldgw, db, cols, N, K, scratch, scratch_floats);
            if (g_grp.on) ts_submit(&a, &w, stream);
            else {
                const TLatPlan lp = tlin_latency_plan(cols, N, Kdx);
                const int nA = lp.gx * lp.gy;
                hipLaunchKernelGGL(tbwd_kernel, dim3(nA + gridW.x * gridW.y), dim3(256), 0, (hipStream_t)stream, a, lp.ksplit, lp.gx, nA, w,
                                   (int)gridW.x, (int)gridW.y);
            }
            STT_HIP(hipGetLastError()); return 0;
        }
    }
    if (int rc = sttode_tlinear(dY, ldy, 1, W, ldw, 1, nullptr, mask, ldm, dX, lddx, cols, N, Kdx, 0, accumulate, stream)) return rc;
    return sttode_twgrad(dY, ldy, X, ldx, xdiv, dW, ldgw, db, cols, N, K, scratch, scratch_floats, stream);
}
