// Latent sets on the device: per agent a set of M = R K points of N(0, I) in zdim dimensions -- a gray-code Sobol sequence
// under a per-agent randomisation (digital shift, or nested uniform scrambling by the Laine-Karras hash), or i.i.d. Philox draws --
// optionally with antithetic halves, the prior mode as sample 0 and a truncated prior, written in the layout inference(z=) /
// inference_reduced(z=) take: z [R][n K][zdim], row = agent K + k, set index m at round m / K, column m % K.
//
// Integer stage in 32-bit wrap-around arithmetic (bit for bit the NumPy restatement of tests/latents_ref.py), value stage in float64:
// u = (x + 0.5) 2^-32, the quantile of u (of its image in the truncated range) by AS241 PPND16 (normal_quantile.hpp), rounded to float32 once.
// Work: agents x chunks of 8 drawn points x quads of dimensions, one item per thread, quads along the lanes.  A chunk starts at a multiple
// of 8, so its first point costs one XOR per set bit of gray(j) and every further point one XOR with a direction number of bit 0, 1 or 2,
// held in registers.  No LDS, no atomics, plain stores; nothing depends on the grid, and an agent's rows depend on (seed, agent index) only.
// The work item and the plan are host and device functions: tests/latents_host.hip loops over the items on the CPU, between guard zones.
#include "../../include/sttode_hip.h"
#include "api_util.hpp"
#include "normal_quantile.hpp"
#include "philox.hpp"
#include <cmath>
#include <cstdint>

namespace {

constexpr int LAT_CHUNK = 8;        // drawn points per thread; a power of two <= 8 keeps ctz(j) of a chunk's inner points below 3
constexpr int LAT_MAX_M = 65536, LAT_MAX_ZDIM = 1024, LAT_DIR_BITS = 30;
constexpr int LAT_MAX_BLOCKS = 1 << 16;

struct LatentArgs {
    float* z; int* bits; const unsigned* dirs;
    int n, K, zdim, Q, nchunks;     // Q quads of dimensions, nchunks chunks of drawn points
    int H, mirrored, c;             // H drawn points; the first `mirrored` of them are written again, negated; c = 1: set index 0 is the zero vector
    int kind, scramble;
    unsigned long long first_agent;
    unsigned k0, k1;
    float t;                        // truncation bound (0: none), w = Phi(t) - Phi(-t)
    double w;
    long long total;
};

// Laine-Karras hash in Burley's form (JCGT 2020): every step is triangular in the bits, so bit i of the result depends on bits <= i of x
__host__ __device__ inline unsigned lk_hash(unsigned x, unsigned s) {
    x += s;
    x ^= x * 0x6c50b47cu;
    x ^= x * 0xb82f1e52u;
    x ^= x * 0xc7afe638u;
    x ^= x * 0x8d22f6e6u;
    return x;
}

template <bool VEC>
__host__ __device__ inline void put(const LatentArgs& A, int al, int m, int d0, int nd, const float (&v)[4], const unsigned (&y)[4]) {
    const int r = m / A.K, k = m - r * A.K;
    const size_t off = (((size_t)r * A.n + al) * A.K + k) * A.zdim + d0;
    if (VEC) {
        *reinterpret_cast<float4*>(A.z + off) = make_float4(v[0], v[1], v[2], v[3]);
        if (A.bits) *reinterpret_cast<int4*>(A.bits + off) = make_int4((int)y[0], (int)y[1], (int)y[2], (int)y[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nd) {
                A.z[off + i] = v[i];
                if (A.bits) A.bits[off + i] = (int)y[i];
            }
    }
}

// one work item: agent it / (nchunks Q), chunk (it / Q) % nchunks, quad it % Q
template <bool VEC>
__host__ __device__ inline void latent_item(const LatentArgs& A, long long it) {
    const int q = (int)(it % A.Q);
    const long long rest = it / A.Q;
    const int chunk = (int)(rest % A.nchunks), al = (int)(rest / A.nchunks);
    const int d0 = 4 * q, nd = A.zdim - d0 < 4 ? A.zdim - d0 : 4, j0 = chunk * LAT_CHUNK;
    const unsigned long long a = A.first_agent + (unsigned long long)al;
    const unsigned a_lo = (unsigned)a, a_hi = (unsigned)(a >> 32);
    unsigned s[4] = {a_lo, a_hi, (unsigned)q, 0u};
    unsigned x[4] = {0u, 0u, 0u, 0u}, v[3][4] = {};
    if (A.kind == 0) {
        if (A.scramble) philox4x32_10(s, A.k0, A.k1);
        const unsigned g = (unsigned)j0 ^ ((unsigned)j0 >> 1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nd) {
                const unsigned* dv = A.dirs + (size_t)(d0 + i) * LAT_DIR_BITS;
                v[0][i] = dv[0] << 2; v[1][i] = dv[1] << 2; v[2][i] = dv[2] << 2;
                for (unsigned gg = g, b = 0; gg; gg >>= 1, ++b)          // j0 < 65536: b <= 16 (bit 2 of gray(j0) is bit 3 of j0)
                    if (gg & 1u) x[i] ^= dv[b] << 2;
            }
    }
    const float zero4[4] = {0.f, 0.f, 0.f, 0.f};
    const unsigned none4[4] = {0u, 0u, 0u, 0u};
    if (A.c && chunk == 0) put<VEC>(A, al, 0, d0, nd, zero4, none4);
#pragma unroll 1
    for (int p = 0; p < LAT_CHUNK; ++p) {                               // (one copy of the value stage: its four quantiles are the ILP)
        const int j = j0 + p;
        if (j >= A.H) break;
        unsigned y[4] = {0u, 0u, 0u, 0u};
        if (A.kind == 0) {
            if (p > 0) {
                const int b = __builtin_ctz((unsigned)p);               // == ctz(j): j0 is a multiple of the chunk
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] ^= b == 0 ? v[0][i] : b == 1 ? v[1][i] : v[2][i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                y[i] = A.scramble == 0 ? x[i] : A.scramble == 1 ? x[i] ^ s[i] : __builtin_bitreverse32(lk_hash(__builtin_bitreverse32(x[i]), s[i]));
        } else {
            y[0] = a_lo; y[1] = a_hi; y[2] = (unsigned)q; y[3] = 1u + (unsigned)j;
            philox4x32_10(y, A.k0, A.k1);
        }
        float zf[4] = {0.f, 0.f, 0.f, 0.f}, neg[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nd) {
                // q = u - 0.5 for u = (x + 0.5) 2^-32, exact in float64.  Truncated: Phi(-t) + u w = 0.5 + q w (Phi(-t) + w / 2 = 0.5): the
                // product keeps the digits of a value near the mode, which a sum next to Phi(-t) would round away
                double q = ((double)y[i] - 2147483647.5) * 2.3283064365386962890625e-10;
                if (A.t > 0.f) q *= A.w;
                float f = (float)stt_ppnd16(q);
                if (A.t > 0.f) f = fminf(fmaxf(f, -A.t), A.t);
                zf[i] = f; neg[i] = -f;
            } else {
                y[i] = 0u;
            }
        put<VEC>(A, al, A.c + j, d0, nd, zf, y);
        if (j < A.mirrored) put<VEC>(A, al, A.c + A.H + j, d0, nd, neg, none4);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void latent_set_kernel(const LatentArgs A) {
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < A.total; it += (long long)gridDim.x * 256) latent_item<VEC>(A, it);
}

// The checks and the geometry of a call: nullptr with A filled, or why the call is refused.
const char* latent_plan(LatentArgs& A, float* z, int* bits, const unsigned* dirs, int n, int K, int R, int zdim, long long first_agent,
                        unsigned long long seed, int kind, int scramble, int antithetic, int center, float truncate) {
    if (!z) return "null pointer (z is required)";
    if (n < 1) return "n must be positive";
    if (K < 1 || R < 1 || K > LAT_MAX_M || R > LAT_MAX_M || (long long)R * K > LAT_MAX_M) return "needs 1 <= M = R K <= 65536 (R, K >= 1)";
    if (zdim < 1 || zdim > LAT_MAX_ZDIM) return "zdim must be in [1, 1024]";
    if (first_agent < 0) return "first_agent must not be negative";
    if (kind != 0 && kind != 1) return "kind must be 0 (Sobol) or 1 (random)";
    if (scramble < 0 || scramble > 2) return "scramble must be 0 (none), 1 (digital shift) or 2 (nested uniform)";
    if ((antithetic != 0 && antithetic != 1) || (center != 0 && center != 1)) return "antithetic and center must be 0 or 1";
    if (!(truncate == 0.f || (std::isfinite(truncate) && truncate >= 0.01f))) return "truncate must be 0 or finite and >= 0.01";
    if (kind == 0 && !dirs) return "null pointer (kind 0 needs dirs, the [zdim][30] direction numbers)";
    const int M = R * K;
    if (center && M < 2) return "center needs M = R K >= 2";
    A = LatentArgs{};
    A.z = z; A.bits = bits; A.dirs = dirs;
    A.n = n; A.K = K; A.zdim = zdim;
    A.c = center;
    const int B = M - center;
    A.H = antithetic ? (B + 1) / 2 : B;
    A.mirrored = B - A.H;
    A.Q = (zdim + 3) / 4;
    A.nchunks = (A.H + LAT_CHUNK - 1) / LAT_CHUNK;
    A.kind = kind; A.scramble = kind == 0 ? scramble : 0;
    A.first_agent = (unsigned long long)first_agent;
    A.k0 = (unsigned)seed; A.k1 = (unsigned)(seed >> 32);
    A.t = truncate;
    if (truncate > 0.f) A.w = std::erf((double)truncate * M_SQRT1_2);          // Phi(t) - Phi(-t)
    A.total = (long long)n * A.nchunks * A.Q;
    return nullptr;
}

// the 16-byte stores need whole quads and aligned bases; everything else takes the scalar stores
bool latent_vec(const LatentArgs& A) { return A.zdim % 4 == 0 && ((uintptr_t)A.z & 15) == 0 && ((uintptr_t)A.bits & 15) == 0; }

}  // namespace

extern "C" int sttode_latent_set(float* z, int* bits, const unsigned* dirs, int n, int K, int R, int zdim, long long first_agent,
                                 unsigned long long seed, int kind, int scramble, int antithetic, int center, float truncate, void* stream) {
    LatentArgs A;
    if (const char* why = latent_plan(A, z, bits, dirs, n, K, R, zdim, first_agent, seed, kind, scramble, antithetic, center, truncate))
        return stt_refuse("sttode_latent_set", why);
    const long long blocks = (A.total + 255) / 256;
    const int grid = (int)(blocks < LAT_MAX_BLOCKS ? blocks : LAT_MAX_BLOCKS);
    if (latent_vec(A)) hipLaunchKernelGGL(latent_set_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(latent_set_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, A);
    STT_HIP(hipGetLastError());
    return 0;
}
