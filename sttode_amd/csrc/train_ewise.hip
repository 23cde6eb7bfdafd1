// Training step, the pieces without a matrix product (family index: train.hip): the decoder's layer-1 input prefix, row copies and
// reductions, the element-wise op codes with their group-mode queue (stt_ew_group, train_group.hpp), LayerNorm forward / backward and
// the gather of the tape rows that carry a gradient.
#include "api_util.hpp"
#include "chain.hpp"
#include "train_group.hpp"

// ---------------------------------------------------------------------------------------------------
// The decoder's layer-1 input prefix of BOTH decompose blocks in one launch: row c = (agent a, sample k) of inp0 / inp1 [n K1, ld] gets
// cat(past_feature[a] (128), z (32)) with z = the posterior draw qz[a] for k = 0 and the prior draw eps[a, k - 1] otherwise
// (model/STTODE.py:322-331, 553-566; the blocks' own state fills columns 160.. later).  Replaces two repeat_interleave copies per block
// and the two that assembled z: six launches of a launch-bound step.
// ---------------------------------------------------------------------------------------------------
__global__ void decoder_inputs_kernel(float* inp0, float* inp1, long ld, const float* pf, long ldpf, const float* qz, const float* eps, int n, int K1,
                                      int pfw, int zd) {
    const int q4 = (pfw + zd) / 4;                                    // float4 pieces of a row's prefix cat(pf [pfw = 2 hidden_dim], z [zdim]): 40 at the defaults
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)n * K1 * q4) return;
    const int f = (int)(id % q4) * 4;
    const long c = id / q4;
    const int a = (int)(c / K1), k = (int)(c % K1);
    const float* src = f < pfw ? pf + (long)a * ldpf + f : (k == 0 ? qz + (long)a * zd : eps + ((long)a * (K1 - 1) + k - 1) * zd) + (f - pfw);
    const f32x4 v = {src[0], src[1], src[2], src[3]};
    st4(inp0 + c * ld + f, v);
    if (inp1) st4(inp1 + c * ld + f, v);
}
extern "C" int sttode_decoder_inputs(float* inp0, float* inp1, long ld, const float* pf, long ldpf, const float* qz, const float* eps, int n,
                                     int K1, int pfw, int zd, void* stream) {
    STT_REQUIRE(inp0 && pf && qz && eps && n > 0 && K1 >= 1 && pfw >= 0 && zd > 0 && pfw % 4 == 0 && zd % 4 == 0 && ld >= pfw + zd && ld % 4 == 0 &&
                ldpf >= pfw, "sttode_decoder_inputs: bad argument (pfw, zd multiples of 4; ld >= pfw + zd)");
    STT_REQUIRE(((size_t)inp0 | (size_t)inp1) % 16 == 0, "sttode_decoder_inputs: inp0 / inp1 must be 16-byte aligned");
    const long tot = (long)n * K1 * ((pfw + zd) / 4);
    hipLaunchKernelGGL(decoder_inputs_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, inp0, inp1, ld, pf, ldpf, qz, eps, n, K1,
                       pfw, zd);
    STT_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// row shuffles
// ---------------------------------------------------------------------------------------------------
__global__ void rows_copy_kernel(float* dst, long ldd, const float* src, long lds, int rows, int width, int div, int mod) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)rows * width) return;
    const int r = (int)(e / width), f = (int)(e % width);
    dst[(long)r * ldd + f] = src[(long)((r / div) % mod) * lds + f];
}
// dst[a, f] (+)= sum_{k<K} src[a*K + k, f]
__global__ void rows_reduce_kernel(float* dst, long ldd, const float* src, long lds, int rows_out, int width, int K, int accumulate) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)rows_out * width) return;
    const int r = (int)(e / width), f = (int)(e % width);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += src[((long)r * K + k) * lds + f];
    float* d = dst + (long)r * ldd + f;
    *d = accumulate ? *d + s : s;
}
extern "C" int sttode_rows_copy(float* dst, long ldd, const float* src, long lds, int rows, int width, int div, int mod, void* stream) {
    STT_REQUIRE(dst && src && rows > 0 && width > 0 && div > 0 && mod > 0, "sttode_rows_copy: bad argument");
    const long tot = (long)rows * width;
    hipLaunchKernelGGL(rows_copy_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dst, ldd, src, lds, rows, width, div, mod);
    STT_HIP(hipGetLastError());
    return 0;
}
extern "C" int sttode_rows_reduce(float* dst, long ldd, const float* src, long lds, int rows_out, int width, int K, int accumulate,
                                  void* stream) {
    STT_REQUIRE(dst && src && rows_out > 0 && width > 0 && K > 0, "sttode_rows_reduce: bad argument");
    const long tot = (long)rows_out * width;
    hipLaunchKernelGGL(rows_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dst, ldd, src, lds, rows_out, width, K, accumulate);
    STT_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// element-wise pieces.  op codes of sttode_train_ewise(op, p0..p5, count, i0, i1, f0):
// ---------------------------------------------------------------------------------------------------
enum {
    EW_MUL = 0,        // p0[i] = p1[i] * p2[i]                                 (dropout mask, gate product)
    EW_AXPY = 1,       // p0[i] += f0 * p1[i]
    EW_GATE_BWD = 2,   // given dout=p0, t=p1 (tanh out), s=p2 (sigmoid out): du=p3 = dout*s*(1-t^2), dv=p4 = dout*t*s*(1-s)
    EW_EULER_FWD = 3,  // p0 = relu(p1 + f0 * p2)
    EW_EULER_BWD = 4,  // d = dout(p0) * (out(p1) > 0): dx(p3) += d ; dy(p4) = f0 * d
    EW_RSAMPLE = 5,    // params p1 [rows, 2*i0] (mu | logvar), eps p2 [rows, i0] -> z p0 = mu + eps * exp(logvar / 2)
    EW_RELU_BWD = 6,   // p0[i] = p1[i] * (p2[i] > 0)
    EW_FILL = 7,       // p0[i] = f0
    EW_CUR_ADD = 9,    // p0[c, d] += p1[c / K, d % 2] with row length i0, K = (int)f0   ("+ cur_location", model/STTODE.py:343-344)
    EW_TANH_BWD = 10,  // p0[i] = p1[i] * (1 - p2[i]^2)      (p2 = tanh output)
    EW_LATENT_BWD = 11,  // sampler.py:51-53: dz=p0, dlogvar=p1, A=p2, eps p3 (mode i0: 0 none | 1 shared [nz] | 2 per agent) -> dA=p4
    EW_SUM_CUR = 12,   // p0[c, d] = p1 + p2 (+ p3[c / K, d % 2] if p3)   row length i0, K = (int)f0  (Decoder.forward :336-344)
    EW_SCALE_ADD = 14,       // p0[i] = f0 * p0[i] + (p1 ? p1[i] : 0)
    EW_AXPY_ROWS = 15,       // p0[r, c] += f0 * p1[r * ld + c], c < width: width = i0 & 0xffff, ld = i0 >> 16 (a column block of a wider matrix)
    EW_EULER_BWD_CAT = 13,   // op 4 reading dout = cat(dx0 | dode) as rows of p0 with leading dimension i0: d = dode * (out(p1) > 0); p3 = dx0 + d; p4 = f0 * d
    EW_RSAMPLE_BWD = 8,  // dz=p0 (in), params p1, eps p2 -> dparams p3 [rows, 2*i0]: dmu += dz ; dlogvar += dz * eps * exp(logvar/2) / 2
};

static __device__ __forceinline__ void ewise_body(int op, float* p0, const float* p1, const float* p2, float* p3, float* p4, long count, int i0,
                                                  float f0, long i) {
    if (i >= count) return;
    switch (op) {
        case EW_MUL: p0[i] = p1[i] * p2[i]; break;
        case EW_AXPY: p0[i] += f0 * p1[i]; break;
        case EW_GATE_BWD: {
            const float d = p0[i], t = p1[i], s = p2[i];
            p3[i] = d * s * (1.0f - t * t);
            p4[i] = d * t * s * (1.0f - s);
        } break;
        case EW_EULER_FWD: p0[i] = fmaxf(p1[i] + f0 * p2[i], 0.f); break;
        case EW_EULER_BWD: {
            const float d = p1[i] > 0.f ? p0[i] : 0.f;
            p3[i] += d;
            p4[i] = f0 * d;
        } break;
        case EW_SCALE_ADD: p0[i] = f0 * p0[i] + (p1 ? p1[i] : 0.f); break;
        case EW_AXPY_ROWS: {
            const int width = i0 & 0xffff, ld = i0 >> 16;
            p0[i] += f0 * p1[(i / width) * ld + i % width];
        } break;
        case EW_EULER_BWD_CAT: {   // i0 = ld | (D << 16); D = 0 means 64 (rounds 3-4 callers)
            const int D = (i0 >> 16) ? (i0 >> 16) : 64, ld = i0 & 0xffff;
            const long r = i / D;
            const int c = (int)(i % D);
            const float d = p1[i] > 0.f ? p0[r * ld + D + c] : 0.f;
            p3[i] = p0[r * ld + c] + d;
            p4[i] = f0 * d;
        } break;
        case EW_RSAMPLE: {
            const long r = i / i0;
            const int d = (int)(i % i0);
            p0[i] = p1[r * 2 * i0 + d] + p2[i] * expf(0.5f * p1[r * 2 * i0 + i0 + d]);
        } break;
        case EW_RELU_BWD: p0[i] = p2[i] > 0.f ? p1[i] : 0.f; break;
        case EW_FILL: p0[i] = f0; break;
        case EW_TANH_BWD: p0[i] = p1[i] * (1.0f - p2[i] * p2[i]); break;
        case EW_LATENT_BWD: {
            // z = A * eps + b, logvar = log(A^2 + 1e-8); f0 = K * nz (row length of A viewed [n, K*nz]), nz = i0 >> 2, mode = i0 & 3
            const int mode = i0 & 3, nz = i0 >> 2;
            const float a = p2[i];
            float e = 0.f;
            if (mode == 1) e = p3[i % nz];
            else if (mode == 2) e = p3[(i / (long)f0) * nz + i % nz];
            p4[i] = p0[i] * e + p1[i] * 2.0f * a / (a * a + 1e-8f);
        } break;
        case EW_SUM_CUR: {
            float v = p1[i] + p2[i];
            if (p3) v += p3[((i / i0) / (int)f0) * 2 + (i % i0) % 2];
            p0[i] = v;
        } break;
        case EW_CUR_ADD: {
            const long c = i / i0;
            p0[i] += p1[(c / (int)f0) * 2 + (i % i0) % 2];
        } break;
        case EW_RSAMPLE_BWD: {
            const long r = i / i0;
            const int d = (int)(i % i0);
            p3[r * 2 * i0 + d] += p0[i];
            p3[r * 2 * i0 + i0 + d] += p0[i] * p2[i] * 0.5f * expf(0.5f * p1[r * 2 * i0 + i0 + d]);
        } break;
    }
}

__global__ void ewise_kernel(int op, float* p0, const float* p1, const float* p2, float* p3, float* p4, long count, int i0, float f0) {
    ewise_body(op, p0, p1, p2, p3, p4, count, i0, f0, (long)blockIdx.x * blockDim.x + threadIdx.x);
}
// up to four independent element-wise pieces in one launch (sttode_tgemm_group: the same piece of the two encoder trunks)
#define EW_MULTI_MAX 4
struct EwProb { float* p0; const float* p1; const float* p2; float* p3; float* p4; long count; int op, i0; float f0; int blk0; };
struct EwMulti { EwProb p[EW_MULTI_MAX]; int n, blocks; };
__global__ void ewise_multi_kernel(EwMulti M) {
#pragma unroll
    for (int k = 0; k < EW_MULTI_MAX; ++k) {
        if (k >= M.n) break;
        const EwProb& e = M.p[k];
        const int last = k + 1 < M.n ? M.p[k + 1 < EW_MULTI_MAX ? k + 1 : k].blk0 : M.blocks;
        if ((int)blockIdx.x >= e.blk0 && (int)blockIdx.x < last)
            ewise_body(e.op, e.p0, e.p1, e.p2, e.p3, e.p4, e.count, e.i0, e.f0, (long)((int)blockIdx.x - e.blk0) * blockDim.x + threadIdx.x);
    }
}
// group mode (sttode_tgemm_group -> stt_ew_group): pieces queued in an open group leave as ONE ewise_multi_kernel launch
// (g_ewq belongs to the calling host thread, like every queue of a group: another thread's calls neither see it nor wait for it)
static thread_local struct { EwMulti M; void* stream; bool on; } g_ewq = {};
static void ew_group_launch() {
    if (g_ewq.M.n == 0) return;
    hipLaunchKernelGGL(ewise_multi_kernel, dim3((unsigned)g_ewq.M.blocks), dim3(256), 0, (hipStream_t)g_ewq.stream, g_ewq.M);
    g_ewq.M.n = 0; g_ewq.M.blocks = 0;
}
int stt_ew_group(int on) {
    if (on < 0) { g_ewq.M.n = 0; g_ewq.M.blocks = 0; }   // error paths: forget what is queued
    ew_group_launch();
    g_ewq.on = on > 0;
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_train_ewise(int op, float* p0, const float* p1, const float* p2, float* p3, float* p4, long count, int i0,
                                  float f0, void* stream) {
    STT_REQUIRE(op >= 0 && op <= EW_AXPY_ROWS && p0 && count > 0, "sttode_train_ewise: bad argument");
    if (g_ewq.on && count <= (1L << 24)) {   // an open group: queued, leaves with the group's other pieces
        EwMulti& M = g_ewq.M;
        if (M.n == EW_MULTI_MAX || (M.n > 0 && g_ewq.stream != stream)) ew_group_launch();
        EwProb& e = M.p[M.n++];
        e.p0 = p0; e.p1 = p1; e.p2 = p2; e.p3 = p3; e.p4 = p4; e.count = count; e.op = op; e.i0 = i0; e.f0 = f0; e.blk0 = M.blocks;
        M.blocks += (int)((count + 255) / 256);
        g_ewq.stream = stream;
        return 0;
    }
    hipLaunchKernelGGL(ewise_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, op, p0, p1, p2, p3, p4, count, i0, f0);
    STT_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// LayerNorm(x + r) over 64 features, one wave per row (lane = feature); backward with per-WG partials
// ---------------------------------------------------------------------------------------------------
static __device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// D = hidden_dim (32 / 64 / 128: LayerNorm over the model dimension, hypertransformer.py:119-120); one wave per row, lane l holds elements
// l, l + 64 (D = 128) or is idle beyond D (D = 32).  D = 64: one element per lane, the sums of rounds 1-4.
template <int D>
__global__ __launch_bounds__(256) void add_ln_fwd_kernel(const float* x, const float* r, const float* gamma, const float* beta,
                                                         float* y, float* xhat, float* rstd, int rows) {
    constexpr int NE = D > 64 ? D / 64 : 1;
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const bool on = lane < D;
    float v[NE], tot = 0.f;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const long o = (long)row * D + lane + 64 * e;
        v[e] = on ? x[o] + (r ? r[o] : 0.f) : 0.f;
        tot += v[e];
    }
    const float mean = wsum(tot) * (1.0f / D);
    float d[NE], sq = 0.f;
#pragma unroll
    for (int e = 0; e < NE; ++e) { d[e] = on ? v[e] - mean : 0.f; sq += d[e] * d[e]; }
    const float rs = 1.0f / sqrtf(wsum(sq) * (1.0f / D) + 1e-5f);
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        if (!on) continue;
        const long o = (long)row * D + lane + 64 * e;
        const float xh = d[e] * rs;
        xhat[o] = xh;
        y[o] = xh * gamma[lane + 64 * e] + beta[lane + 64 * e];
    }
    if (lane == 0) rstd[row] = rs;
}

// dsum = grad wrt (x + r); dgamma / dbeta accumulated deterministically: WG g sums its rows, a single last pass adds the
// per-WG partials in order (grid is small: rows <= a few thousand).
template <int D>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* dy, const float* xhat, const float* rstd, const float* gamma,
                                                     float* dsum, float* part, int rows, int rows_per_wg, float* dgamma, float* dbeta) {
    constexpr int NE = D > 64 ? D / 64 : 1;
    __shared__ float sg[4][NE * 64], sb[4][NE * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * rows_per_wg, r1 = min(r0 + rows_per_wg, rows);
    const bool on = lane < D;
    float ag[NE], ab[NE], g[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) { ag[e] = ab[e] = 0.f; g[e] = on ? gamma[lane + 64 * e] : 0.f; }
    for (int row = r0 + wave; row < r1; row += 4) {
        float dd[NE], xh[NE], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const long o = (long)row * D + lane + 64 * e;
            dd[e] = on ? dy[o] : 0.f;
            xh[e] = on ? xhat[o] : 0.f;
            ag[e] += dd[e] * xh[e];
            ab[e] += dd[e];
            const float dh = dd[e] * g[e];
            s1 += dh;
            s2 += dh * xh[e];
        }
        const float m1 = wsum(s1) * (1.0f / D), m2 = wsum(s2) * (1.0f / D);
#pragma unroll
        for (int e = 0; e < NE; ++e)
            if (on) dsum[(long)row * D + lane + 64 * e] = rstd[row] * (dd[e] * g[e] - m1 - xh[e] * m2);
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) { sg[wave][lane + 64 * e] = ag[e]; sb[wave][lane + 64 * e] = ab[e]; }
    __syncthreads();
    if (wave == 0 && on) {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int c = lane + 64 * e;
            const float tg = ((sg[0][c] + sg[1][c]) + sg[2][c]) + sg[3][c], tb = ((sb[0][c] + sb[1][c]) + sb[2][c]) + sb[3][c];
            if (dgamma) {   // a single workgroup (rows <= 64: scene sizes): no partials, no second launch
                dgamma[c] += tg;
                dbeta[c] += tb;
            } else {
                part[(long)blockIdx.x * 2 * D + c] = tg;
                part[(long)blockIdx.x * 2 * D + D + c] = tb;
            }
        }
    }
}
__global__ void ln_bwd_reduce_kernel(const float* part, int G, float* dgamma, float* dbeta, int D) {
    const int t = threadIdx.x;  // 2 D threads
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += part[(long)g * 2 * D + t];
    if (t < D) dgamma[t] += s;
    else dbeta[t - D] += s;
}

#define LN_DISPATCH(D_, CALL)                                                                          \
    do {                                                                                               \
        if ((D_) == 64) { constexpr int DD = 64; CALL; }                                               \
        else if ((D_) == 32) { constexpr int DD = 32; CALL; }                                          \
        else if ((D_) == 128) { constexpr int DD = 128; CALL; }                                        \
        else STT_REQUIRE(false, "LayerNorm kernels: hidden_dim must be 32, 64 or 128");                \
    } while (0)

extern "C" int sttode_add_ln_fwd(const float* x, const float* r, const float* gamma, const float* beta, float* y, float* xhat,
                                 float* rstd, int rows, int D, void* stream) {
    STT_REQUIRE(x && gamma && beta && y && xhat && rstd && rows > 0, "sttode_add_ln_fwd: bad argument");
    LN_DISPATCH(D, hipLaunchKernelGGL(add_ln_fwd_kernel<DD>, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, r, gamma, beta, y, xhat, rstd, rows));
    STT_HIP(hipGetLastError());
    return 0;
}
extern "C" int sttode_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dsum, float* dgamma,
                             float* dbeta, int rows, int D, float* scratch, long scratch_floats, void* stream) {
    STT_REQUIRE(dy && xhat && rstd && gamma && dsum && dgamma && dbeta && scratch && rows > 0, "sttode_ln_bwd: bad argument");
    // one workgroup up to 64 rows (scene sizes: no partials, no second launch); beyond that 16 rows per workgroup (round 5: 6 workgroups for the
    // 352 rows of an NBA-size step took 11 us; the reduction launch adds the per-workgroup partials in order either way)
    int G = rows <= 64 ? 1 : (rows + 15) / 16;
    if (G > 256) G = 256;
    STT_REQUIRE(scratch_floats >= (long)G * 2 * D, "sttode_ln_bwd: scratch too small");
    const int rpw = (rows + G - 1) / G;
    LN_DISPATCH(D, hipLaunchKernelGGL(ln_bwd_kernel<DD>, dim3(G), dim3(256), 0, (hipStream_t)stream, dy, xhat, rstd, gamma, dsum, scratch, rows, rpw,
                                      G == 1 ? dgamma : nullptr, G == 1 ? dbeta : nullptr));
    if (G > 1) hipLaunchKernelGGL(ln_bwd_reduce_kernel, dim3(1), dim3(2 * D), 0, (hipStream_t)stream, scratch, G, dgamma, dbeta, D);
    STT_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// The rows of the decoder's tape that carry a gradient (sttode_loss_objective_live): per agent, of its K1 trajectory columns, sample 0 and
// sample best[a] -> rows 2 a and 2 a + 1 of a compact copy.  Every tensor of the tape is rows of `row` floats, `outer` planes of them
// (the GRU's per-step planes [T][columns][..]); up to STT_GATHER_MAX tensors per launch, one workgroup per (tensor, plane, output row).
// ---------------------------------------------------------------------------------------------------
#define STT_GATHER_MAX 32
struct GatherItem { const float* src; float* dst; long src_plane; long dst_plane; int row; int outer; };   // planes in floats
struct GatherArgs { GatherItem it[STT_GATHER_MAX]; int blk0[STT_GATHER_MAX + 1]; int count; const int* best; int n, K1; };
__global__ __launch_bounds__(128) void live_rows_gather_kernel(GatherArgs g) {
    int p = 0;
    while (p + 1 < g.count && (int)blockIdx.x >= g.blk0[p + 1]) ++p;
    const GatherItem& it = g.it[p];
    const int local = (int)blockIdx.x - g.blk0[p], rows = 2 * g.n;
    const int o = local / rows, r = local % rows, a = r >> 1;
    int sidx = (r & 1) ? g.best[a] : 0;
    sidx = sidx < 0 ? 0 : (sidx >= g.K1 ? g.K1 - 1 : sidx);     // (a `best` nobody wrote must not turn into an out-of-bounds read)
    const float* src = it.src + (long)o * it.src_plane + ((long)a * g.K1 + sidx) * it.row;
    float* dst = it.dst + (long)o * it.dst_plane + (long)r * it.row;
    if ((it.row & 3) == 0 && ((((size_t)src) | ((size_t)dst)) & 15) == 0) {
        for (int i = threadIdx.x; i < it.row / 4; i += 128) reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[i];
    } else {
        for (int i = threadIdx.x; i < it.row; i += 128) dst[i] = src[i];
    }
}
extern "C" int sttode_live_rows_gather(const void* items_, int count, const int* best, int n, int K1, void* stream) {
    const GatherItem* items = (const GatherItem*)items_;
    STT_REQUIRE(items && best && count > 0 && count <= STT_GATHER_MAX && n > 0 && K1 >= 2, "sttode_live_rows_gather: null pointer or bad counts (at most 32 tensors)");
    GatherArgs g;
    g.count = count; g.best = best; g.n = n; g.K1 = K1;
    long blocks = 0;
    for (int i = 0; i < count; ++i) {
        STT_REQUIRE(items[i].src && items[i].dst && items[i].row > 0 && items[i].outer > 0, "sttode_live_rows_gather: bad item");
        g.it[i] = items[i];
        g.blk0[i] = (int)blocks;
        blocks += (long)items[i].outer * 2 * n;
    }
    STT_REQUIRE(blocks < (1L << 31), "sttode_live_rows_gather: too many rows");
    g.blk0[count] = (int)blocks;
    hipLaunchKernelGGL(live_rows_gather_kernel, dim3((unsigned)blocks), dim3(128), 0, (hipStream_t)stream, g);
    STT_HIP(hipGetLastError());
    return 0;
}
