// Poincare-ball primitives (hyptorch/pmath.py) and Oblique-manifold primitives (core/manifolds/oblique.py)
// as a stand-alone HIP op library.  None of these is called by the STTODE model path: parity is
// op-level, against vectors produced by the reference's own functions (tests/golden/pmath.npz, ops.npz).
//
// Row-wise ops: ONE WAVE PER ROW (4 rows per 256-thread block), lanes stride the feature dim with coalesced loads,
// the three row reductions (|x|^2, |y|^2, <x,y>) are a single pass + wavefront xor-shuffles; a second pass writes
// the vector result (or lane 0 the scalar).  HBM-bound: 1 read of each operand + 1 write.  The reference's epsilons
// and clamps are kept verbatim (cited per op).
#include "api_util.hpp"
#include "pmath_curv.hpp"
#include <cmath>

enum PmathOp {
    OP_PROJECT = 0, OP_LAMBDA_X, OP_MOBIUS_ADD, OP_DIST, OP_DIST0, OP_EXPMAP, OP_EXPMAP0, OP_LOGMAP, OP_LOGMAP0, OP_P2K, OP_K2P,
    OP_LORENZ, OP_OBL_PROJ, OP_MATVEC_FIN, OP_PMEAN_PREP, OP_COUNT
};

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float tanh_clamped(float x) { return tanhf(fminf(fmaxf(x, -15.0f), 15.0f)); }  // pmath.py:11-12
__device__ __forceinline__ float artanh_(float x) {                                                        // pmath.py:16-22
    x = fminf(fmaxf(x, -1.0f + 1e-5f), 1.0f - 1e-5f);
    return (logf(1.0f + x) - logf(1.0f - x)) * 0.5f;
}
__device__ __forceinline__ float arsinh_(float x) { return logf(fmaxf(x + sqrtf(1.0f + x * x), 1e-5f)); }    // pmath.py:51-55

// mobius_add(a, b)_i for a = sx*x (sx = +-1) given the row scalars of the SIGNED operand (pmath.py:171-177)
struct MobCoef { float ca, cb, den; };
__device__ __forceinline__ MobCoef mob_coef(float a2, float b2, float ab, float c) {
    MobCoef m;
    m.ca = 1.0f + 2.0f * c * ab + c * b2;
    m.cb = 1.0f - c * a2;
    m.den = 1.0f + 2.0f * c * ab + c * c * a2 * b2 + 1e-5f;
    return m;
}

__global__ __launch_bounds__(256) void pmath_row_kernel(int op, const float* __restrict__ x, const float* __restrict__ y,
                                                        float* __restrict__ out, float* __restrict__ out2, int rows, int d, float cv,
                                                        const float* __restrict__ cp) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float c = cp ? *cp : cv;   // the curvature: a value of the launch, or one float on the device (the _c entry points)
    const float* xr = x + (size_t)r * d;
    const float* yr = y ? y + (size_t)r * d : nullptr;
    float x2 = 0.f, y2 = 0.f, xy = 0.f;
    for (int i = lane; i < d; i += 64) {
        const float a = xr[i];
        x2 += a * a;
        if (yr) { const float b = yr[i]; y2 += b * b; xy += a * b; }
    }
    x2 = wsum(x2); y2 = wsum(y2); xy = wsum(xy);
    const float sc = sqrtf(c);
    float* o = out + (size_t)r * d;
    switch (op) {
        case OP_PROJECT: {  // pmath.py:98-103
            const float norm = fmaxf(sqrtf(x2), 1e-5f), maxnorm = (1.0f - 1e-3f) / sc;
            for (int i = lane; i < d; i += 64) o[i] = norm > maxnorm ? xr[i] / norm * maxnorm : xr[i];
        } break;
        case OP_LAMBDA_X:  // pmath.py:128-129
            if (lane == 0) out[r] = 2.0f / (1.0f - c * x2);
            break;
        case OP_MOBIUS_ADD: {
            const MobCoef m = mob_coef(x2, y2, xy, c);
            for (int i = lane; i < d; i += 64) o[i] = (m.ca * xr[i] + m.cb * yr[i]) / m.den;
        } break;
        case OP_DIST:      // pmath.py:205-208 : artanh(sqrt_c |(-x) (+) y|) * 2 / sqrt_c
        case OP_LOGMAP: {  // pmath.py:334-339
            const MobCoef m = mob_coef(x2, y2, -xy, c);
            float s2 = 0.f;
            for (int i = lane; i < d; i += 64) { const float v = (m.ca * (-xr[i]) + m.cb * yr[i]) / m.den; s2 += v * v; }
            const float sn = sqrtf(wsum(s2));
            if (op == OP_DIST) {
                if (lane == 0) out[r] = artanh_(sc * sn) * 2.0f / sc;
            } else {
                const float lam = 2.0f / (1.0f - c * x2);
                const float k = 2.0f / sc / lam * artanh_(sc * sn);
                for (int i = lane; i < d; i += 64) o[i] = k * ((m.ca * (-xr[i]) + m.cb * yr[i]) / m.den) / sn;
            }
        } break;
        case OP_DIST0:  // pmath.py:231-234
            if (lane == 0) out[r] = artanh_(sc * sqrtf(x2)) * 2.0f / sc;
            break;
        case OP_EXPMAP: {  // pmath.py:268-277 : x (+) tanh(sqrt_c/2 * lambda_x * |u|) u / (sqrt_c |u|)   (u passed as y)
            const float un = fmaxf(sqrtf(y2), 1e-5f);
            const float lam = 2.0f / (1.0f - c * x2);
            const float t = tanh_clamped(sc / 2.0f * lam * un);
            const float s = t / (sc * un);  // second_term = s * u (elementwise: t * u / (sc*un))
            const MobCoef m = mob_coef(x2, s * s * y2, s * xy, c);
            for (int i = lane; i < d; i += 64) o[i] = (m.ca * xr[i] + m.cb * (t * yr[i] / (sc * un))) / m.den;
        } break;
        case OP_EXPMAP0: {  // pmath.py:300-304
            const float un = fmaxf(sqrtf(x2), 1e-5f);
            const float t = tanh_clamped(sc * un);
            for (int i = lane; i < d; i += 64) o[i] = t * xr[i] / (sc * un);
        } break;
        case OP_LOGMAP0: {  // pmath.py:365-368
            const float yn = fmaxf(sqrtf(x2), 1e-5f);
            const float a = artanh_(sc * yn);
            for (int i = lane; i < d; i += 64) o[i] = xr[i] / yn / sc * a;
        } break;
        case OP_P2K:  // pmath.py:440-442
            for (int i = lane; i < d; i += 64) o[i] = 2.0f * xr[i] / (1.0f + c * x2);
            break;
        case OP_K2P:  // pmath.py:445-447
            for (int i = lane; i < d; i += 64) o[i] = xr[i] / (1.0f + sqrtf(1.0f - c * x2));
            break;
        case OP_LORENZ:  // pmath.py:450-469
            if (lane == 0) out[r] = 1.0f / sqrtf(1.0f - c * x2);
            break;
        case OP_OBL_PROJ:  // core/manifolds/oblique.py:15-16
            for (int i = lane; i < d; i += 64) o[i] = xr[i] / sqrtf(x2);
            break;
        case OP_MATVEC_FIN: {  // pmath.py:399-408 ; x = mx row [d], y = original x row passed via out2-stride trick (see host)
            // here: xr = mx row (length d), yr = nullptr; out2 holds |x| per row
            const float xn = fmaxf(out2[r], 1e-5f);
            const float mxn = sqrtf(x2);
            const float t = tanh_clamped(mxn / xn * artanh_(sc * xn));
            const bool zero = x2 == 0.0f;
            // res then _project
            float r2 = 0.f;
            for (int i = lane; i < d; i += 64) { const float v = zero ? 0.f : t * xr[i] / (mxn * sc); r2 += v * v; }
            const float norm = fmaxf(sqrtf(wsum(r2)), 1e-5f), maxnorm = (1.0f - 1e-3f) / sc;
            for (int i = lane; i < d; i += 64) {
                const float v = zero ? 0.f : t * xr[i] / (mxn * sc);
                o[i] = norm > maxnorm ? v / norm * maxnorm : v;
            }
        } break;
        case OP_PMEAN_PREP: {  // pmath.py:472-476 : xk = p2k(x); lam = lorenz(xk); out = lam * xk, out2[r] = lam
            // 1 - c|xk|^2 = ((1 - c|x|^2) / (1 + c|x|^2))^2 is ~1e-6 for rows on the ball boundary: formed from fp32 Klein coordinates
            // it is only good to a few percent (the reference's own fp32 result is ~1e-3..6e-3 off the exact value there).  The Lorenz
            // factor is therefore taken in closed form, lam = (1 + c|x|^2) / (1 - c|x|^2), from a float64 sum of squares.
            double x2d = 0.;
            for (int i = lane; i < d; i += 64) { const double a = xr[i]; x2d += a * a; }
#pragma unroll
            for (int ofs = 32; ofs > 0; ofs >>= 1) x2d += __shfl_xor(x2d, ofs, 64);
            const double dend = 1.0 + (double)c * x2d;
            const double lamd = dend / (1.0 - (double)c * x2d);
            for (int i = lane; i < d; i += 64) o[i] = (float)(lamd * (2.0 * (double)xr[i] / dend));
            if (lane == 0) out2[r] = (float)lamd;
        } break;
    }
}

// poincare_mean tail (pmath.py:476-479): mean = sum_r(lam*xk) / sum_r(lam) ; k2p(mean).  One block.
__global__ __launch_bounds__(1024) void pmean_fin_kernel(const float* __restrict__ yl, const float* __restrict__ lam,
                                                         float* __restrict__ out, int rows, int d, float c) {
    __shared__ float red[16];
    __shared__ float tot;
    float L = 0.f;
    for (int r = 0; r < rows; ++r) L += lam[r];
    float part = 0.f;
    for (int i = threadIdx.x; i < d; i += blockDim.x) {
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s += yl[(size_t)r * d + i];
        const float m = s / L;
        out[i] = m;
        part += m * m;
    }
    part = wsum(part);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
        tot = t;
    }
    __syncthreads();
    const float den = 1.0f + sqrtf(1.0f - c * tot);
    for (int i = threadIdx.x; i < d; i += blockDim.x) out[i] = out[i] / den;
}

// poincare_mean at a general shape: x is [outer, R, inner] rows of length d and the mean runs over R, with no permuted
// copy.  ONE BLOCK PER GROUP (o, n), running pmean_fin_kernel's body -- the same thread count, the same sums in the same order -- at the
// group's offset with the row stride inner d, so a group's result is bitwise that of the 2-D call on its rows.  The curvature as in
// pmath_row_kernel.  klein / lsum (each may be NULL): the Klein mean before k2p [groups, d] and L = sum of the Lorentz factors [groups].
__global__ __launch_bounds__(1024) void pmean_seg_fin_kernel(const float* __restrict__ yl, const float* __restrict__ lam,
                                                             float* __restrict__ out, float* __restrict__ klein, float* __restrict__ lsum, int R,
                                                             int inner, int d, float cv, const float* __restrict__ cp) {
    __shared__ float red[16];
    __shared__ float tot;
    const float c = cp ? *cp : cv;
    const size_t o = blockIdx.x / inner, n = blockIdx.x % inner;
    const size_t row0 = o * R * inner + n;              // the group's first row; its rows are row0 + r inner
    yl += row0 * d;
    lam += row0;
    out += (size_t)blockIdx.x * d;
    const size_t rs = (size_t)inner * d;
    float L = 0.f;
    for (int r = 0; r < R; ++r) L += lam[(size_t)r * inner];
    float part = 0.f;
    for (int i = threadIdx.x; i < d; i += blockDim.x) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += yl[(size_t)r * rs + i];
        const float m = s / L;
        out[i] = m;
        if (klein) klein[(size_t)blockIdx.x * d + i] = m;
        part += m * m;
    }
    if (lsum && threadIdx.x == 0) lsum[blockIdx.x] = L;
    part = wsum(part);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
        tot = t;
    }
    __syncthreads();
    const float den = 1.0f + sqrtf(1.0f - c * tot);
    for (int i = threadIdx.x; i < d; i += blockDim.x) out[i] = out[i] / den;
}

// elementwise scalars: tanh (clamped), artanh, arsinh
__global__ void pmath_scalar_kernel(int which, const float* __restrict__ x, float* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    switch (which) {
        case 0: out[i] = tanh_clamped(v); break;
        case 1: out[i] = artanh_(v); break;
        case 2: out[i] = arsinh_(v); break;
        case 3: {  // d artanh / dx at the clamped input (Artanh.backward, hyptorch/pmath.py:25-27)
            const float xc = fminf(fmaxf(v, -1.0f + 1e-5f), 1.0f - 1e-5f);
            out[i] = 1.0f / (1.0f - __fmul_rn(xc, xc));   // no fma contraction: 1 - x^2 cancels to ~2e-5 at the clamp
        } break;
        default: out[i] = 1.0f / sqrtf(1.0f + __fmul_rn(v, v)); break;   // d arsinh / dx (Arsinh.backward, :57-60)
    }
}

// RiemannianGradient.backward (hyptorch/pmath.py:39-45): out[r, :] = g[r, :] * (1 - c |x_r|^2)^2 / 4
__global__ void riemannian_grad_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ out, int rows, int d, float c) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float n2 = 0.f;
    for (int i = 0; i < d; ++i) { const float a = x[(size_t)r * d + i]; n2 += a * a; }
    const float t = 1.0f - c * n2;
    const float sc = t * t * 0.25f;
    for (int i = 0; i < d; ++i) out[(size_t)r * d + i] = g[(size_t)r * d + i] * sc;
}

// mx[r][o] = <x[r], m[o]>   (mobius_matvec front half)
__global__ void rowdot_kernel(const float* __restrict__ x, const float* __restrict__ m, float* __restrict__ mx, float* __restrict__ xnorm,
                              int rows, int d, int O) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)rows * O) return;
    const int r = idx / O, o = idx % O;
    float s = 0.f, n2 = 0.f;
    for (int i = 0; i < d; ++i) { const float a = x[(size_t)r * d + i]; s += a * m[(size_t)o * d + i]; n2 += a * a; }
    mx[idx] = s;
    if (o == 0) xnorm[r] = sqrtf(n2);
}

// pairwise kernels: one thread per (p, q).  which: 0 dist_matrix [P,R]; 1 mobius_addition_batch [P,R,D]; 2 hyperbolic_softmax
__global__ void pmath_pair_kernel(int which, const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ A,
                                  float* __restrict__ out, int P, int R, int d, float cv, const float* __restrict__ cp) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)P * R) return;
    const float c = cp ? *cp : cv;   // as in pmath_row_kernel
    const int p = idx / R, q = idx % R;
    const float* xr = x + (size_t)p * d;
    const float* yr = y + (size_t)q * d;
    const float sgn = (which == 1) ? 1.0f : -1.0f;  // dist_matrix / hyperbolic_softmax call batch(-x, y)
    // Row scalars and the Moebius sum are formed in float64 and rounded once: 1 - c|x|^2 cancels catastrophically for rows on the ball
    // boundary (|x|^2 -> (1-1e-3)^2 / c), where a 1-ulp error of an fp32 sum of squares becomes 5e-5 relative in the coefficient and
    // is amplified again by artanh's slope (~500).  The fp32 result of the reference is only defined to that level there; the
    // float64 path keeps this kernel within 1e-6 of the exact value of the same fp32 inputs (tests: float64 yardstick).
    double x2 = 0., y2 = 0., xy = 0.;
    for (int i = 0; i < d; ++i) { const double a = sgn * xr[i], b = yr[i]; x2 += a * a; y2 += b * b; xy += a * b; }
    const double cd = c;
    const double ca = 1.0 + 2.0 * cd * xy + cd * y2, cb = 1.0 - cd * x2;                 // pmath.py:416-427
    const double den = 1.0 + 2.0 * cd * xy + cd * cd * x2 * y2 + (double)1e-5f;
    if (which == 1) {
        for (int i = 0; i < d; ++i) out[idx * d + i] = (float)((ca * (double)(sgn * xr[i]) + cb * (double)yr[i]) / den);
        return;
    }
    double s2 = 0., sa = 0., a2 = 0.;
    for (int i = 0; i < d; ++i) {
        const double v = (ca * (double)(-xr[i]) + cb * (double)yr[i]) / den;
        s2 += v * v;
        if (which == 2) { const double av = A[(size_t)p * d + i]; sa += v * av; a2 += av * av; }
    }
    const double sc = sqrt(cd);
    if (which == 0) {
        double u = sc * sqrt(s2);
        u = fmin(fmax(u, -1.0 + (double)1e-5f), 1.0 - (double)1e-5f);                     // Artanh clamp, pmath.py:19
        out[idx] = (float)(2.0 / sc * 0.5 * (log1p(u) - log1p(-u)));                     // pmath.py:482-493
    } else {
        // _hyperbolic_softmax (pmath.py:430-437): x = P (classes, rows p), y = X (batch, rows q); result [B, C] = out[q][p]
        const double an = sqrt(a2);
        const double lam = 2.0 / (1.0 - cd * x2);
        const double k = lam * an / sc;
        const double num = 2.0 * sc * sa;
        const double dn = an * (1.0 - cd * s2);
        const double t = num / dn;
        out[(size_t)q * P + p] = (float)(k * log(fmax(t + sqrt(1.0 + t * t), (double)1e-5f)));
    }
}

// Oblique.dist(p1, p2) = acos(clamp(p2 @ p1^T)) -> [batch, rows(p2), rows(p1)]   (core/manifolds/oblique.py:36-43)
__global__ void oblique_dist_kernel(const float* __restrict__ p1, const float* __restrict__ p2, float* __restrict__ out, int nb, int n1,
                                    int n2, int d) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)nb * n2 * n1) return;
    const int j = idx % n1, i = (idx / n1) % n2, b = idx / ((long)n1 * n2);
    const float* a = p2 + ((size_t)b * n2 + i) * d;
    const float* q = p1 + ((size_t)b * n1 + j) * d;
    float s = 0.f;
    for (int k = 0; k < d; ++k) s += a[k] * q[k];
    out[idx] = acosf(fminf(fmaxf(s, -1.0f + 1e-4f), 1.0f - 1e-4f));
}

// ---------------------------------------------------------------------------------------------------
// One host function per operation for its two exported forms (pmath_curv.hpp).  The device form: c_dev points to ONE float
// that the kernels read, so a trainable curvature costs no host read and the call can be captured.  The same kernels, the same
// arithmetic: for *c_dev == v the results are bitwise those of the float form at v.  The value cannot be checked here, so c > 0 is a rule
// of the float form alone; the device form has the row ops 0..11 only (Oblique.proj has no curvature, 13/14 are internal).
static int pmath_rowop(const char* who, int op, const float* x, const float* y, float* out, float* out2, int rows, int d, Curv cv,
                       void* stream) {
    PM_REQUIRE_CURV();
    if (cv.dev) PM_REQUIRE(op >= 0 && op < OP_OBL_PROJ, "unknown op, or one without a device-curvature form");
    else PM_REQUIRE(op >= 0 && op < OP_COUNT, "unknown op");
    PM_REQUIRE(x && out && rows > 0 && d > 0, "null pointer or empty shape");
    const bool needs_y = op == OP_MOBIUS_ADD || op == OP_DIST || op == OP_LOGMAP || op == OP_EXPMAP;
    PM_REQUIRE(!needs_y || y, "this op needs a second operand");
    PM_REQUIRE((op != OP_MATVEC_FIN && op != OP_PMEAN_PREP) || out2, "this op needs the out2 buffer");
    PM_REQUIRE(cv.dev || cv.c > 0.f || op == OP_OBL_PROJ, "curvature c must be positive");
    hipLaunchKernelGGL(pmath_row_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, op, x, needs_y ? y : nullptr, out, out2,
                       rows, d, cv.c, cv.c_dev);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_pmath_rowop(int op, const float* x, const float* y, float* out, float* out2, int rows, int d, float c,
                                  void* stream) {
    return pmath_rowop("sttode_pmath_rowop", op, x, y, out, out2, rows, d, curv_float(c), stream);
}

extern "C" int sttode_pmath_rowop_c(int op, const float* x, const float* y, float* out, float* out2, int rows, int d, const float* c_dev,
                                    void* stream) {
    return pmath_rowop("sttode_pmath_rowop_c", op, x, y, out, out2, rows, d, curv_dev(c_dev), stream);
}

extern "C" int sttode_pmath_scalar(int which, const float* x, float* out, long n, void* stream) {
    STT_REQUIRE(x && out && n > 0 && which >= 0 && which <= 4, "sttode_pmath_scalar: bad arguments");
    hipLaunchKernelGGL(pmath_scalar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, which, x, out, n);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_pmath_riemannian_grad(const float* x, const float* g, float* out, int rows, int d, float c, void* stream) {
    STT_REQUIRE(x && g && out && rows > 0 && d > 0, "sttode_pmath_riemannian_grad: bad arguments");
    hipLaunchKernelGGL(riemannian_grad_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, g, out, rows, d, c);
    STT_HIP(hipGetLastError());
    return 0;
}

static int pmath_matvec(const char* who, const float* m, const float* x, float* mx_ws, float* xnorm_ws, float* out, int rows, int d, int O,
                        Curv cv, void* stream) {
    PM_REQUIRE_CURV();
    PM_REQUIRE(m && x && mx_ws && xnorm_ws && out && rows > 0 && d > 0 && O > 0 && (cv.dev || cv.c > 0.f), "bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const long tot = (long)rows * O;
    hipLaunchKernelGGL(rowdot_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, x, m, mx_ws, xnorm_ws, rows, d, O);
    hipLaunchKernelGGL(pmath_row_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, (int)OP_MATVEC_FIN, (const float*)mx_ws,
                       (const float*)nullptr, out, xnorm_ws, rows, O, cv.c, cv.c_dev);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_pmath_matvec(const float* m, const float* x, float* mx_ws, float* xnorm_ws, float* out, int rows, int d, int O,
                                   float c, void* stream) {
    return pmath_matvec("sttode_pmath_matvec", m, x, mx_ws, xnorm_ws, out, rows, d, O, curv_float(c), stream);
}

extern "C" int sttode_pmath_matvec_c(const float* m, const float* x, float* mx_ws, float* xnorm_ws, float* out, int rows, int d, int O,
                                     const float* c_dev, void* stream) {
    return pmath_matvec("sttode_pmath_matvec_c", m, x, mx_ws, xnorm_ws, out, rows, d, O, curv_dev(c_dev), stream);
}

static int pmath_pair(const char* who, int which, const float* x, const float* y, const float* A, float* out, int P, int R, int d, Curv cv,
                      void* stream) {
    PM_REQUIRE_CURV();
    PM_REQUIRE(x && y && out && P > 0 && R > 0 && d > 0 && (cv.dev || cv.c > 0.f) && which >= 0 && which <= 2, "bad arguments");
    PM_REQUIRE(which != 2 || A, "hyperbolic_softmax needs A");
    const long tot = (long)P * R;
    hipLaunchKernelGGL(pmath_pair_kernel, dim3((unsigned)((tot + 127) / 128)), dim3(128), 0, (hipStream_t)stream, which, x, y, A, out, P, R,
                       d, cv.c, cv.c_dev);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_pmath_pair(int which, const float* x, const float* y, const float* A, float* out, int P, int R, int d, float c,
                                 void* stream) {
    return pmath_pair("sttode_pmath_pair", which, x, y, A, out, P, R, d, curv_float(c), stream);
}

extern "C" int sttode_pmath_pair_c(int which, const float* x, const float* y, const float* A, float* out, int P, int R, int d,
                                   const float* c_dev, void* stream) {
    return pmath_pair("sttode_pmath_pair_c", which, x, y, A, out, P, R, d, curv_dev(c_dev), stream);
}

extern "C" int sttode_pmath_mean(const float* x, float* yl_ws, float* lam_ws, float* out, int rows, int d, float c, void* stream) {
    STT_REQUIRE(x && yl_ws && lam_ws && out && rows > 0 && d > 0 && c > 0.f, "sttode_pmath_mean: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pmath_row_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, (int)OP_PMEAN_PREP, x, (const float*)nullptr, yl_ws, lam_ws,
                       rows, d, c, (const float*)nullptr);
    hipLaunchKernelGGL(pmean_fin_kernel, dim3(1), dim3(1024), 0, s, (const float*)yl_ws, (const float*)lam_ws, out, rows, d, c);
    STT_HIP(hipGetLastError());
    return 0;
}

// poincare_mean over the middle dimension of x [outer, R, inner, d] -> out [outer, inner, d].  The curvature: *c_dev when c_dev is given
// (never checked, as the other _c forms), else c.
extern "C" int sttode_pmath_mean_seg(const float* x, float* yl_ws, float* lam_ws, float* out, float* klein, float* lsum, int outer, int R,
                                     int inner, int d, float c, const float* c_dev, void* stream) {
    STT_REQUIRE(x && yl_ws && lam_ws && out, "sttode_pmath_mean_seg: null pointer");
    STT_REQUIRE(outer > 0 && R > 0 && inner > 0 && d > 0, "sttode_pmath_mean_seg: empty shape");
    STT_REQUIRE((long)outer * R * inner <= 0x7fffffffL, "sttode_pmath_mean_seg: more than 2^31 - 1 rows");
    STT_REQUIRE(c_dev || (c > 0.f && std::isfinite(c)), "sttode_pmath_mean_seg: curvature c must be positive and finite");
    hipStream_t s = (hipStream_t)stream;
    const int rows = outer * R * inner;
    hipLaunchKernelGGL(pmath_row_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, (int)OP_PMEAN_PREP, x, (const float*)nullptr, yl_ws, lam_ws,
                       rows, d, c, c_dev);
    hipLaunchKernelGGL(pmean_seg_fin_kernel, dim3((unsigned)(outer * inner)), dim3(1024), 0, s, (const float*)yl_ws, (const float*)lam_ws, out,
                       klein, lsum, R, inner, d, c, c_dev);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_oblique_dist(const float* p1, const float* p2, float* out, int nb, int n1, int n2, int d, void* stream) {
    STT_REQUIRE(p1 && p2 && out && nb > 0 && n1 > 0 && n2 > 0 && d > 0, "sttode_oblique_dist: bad arguments");
    const long tot = (long)nb * n1 * n2;
    hipLaunchKernelGGL(oblique_dist_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p1, p2, out, nb, n1, n2, d);
    STT_HIP(hipGetLastError());
    return 0;
}
