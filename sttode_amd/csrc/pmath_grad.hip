// Backward passes of the Poincare-ball primitives of pmath.hip (hyptorch/pmath.py): one fused kernel per operation, against the few dozen
// autograd nodes -- and their live intermediates -- that the reference builds per call.
//
// Every row-op result is out = alpha x + beta y with alpha, beta functions of the row scalars p = (|x|^2, |y|^2, <x,y>) and c (dist / logmap:
// |(-x) (+) y|^2 = A^2 p1 - 2 A B p3 + B^2 p2 is itself a closed form in p), or a scalar s(p).  The vector-Jacobian product is therefore
//     gx = alpha g + 2 x L1 + y L3,   gy = beta g + 2 y L2 + x L3,   L_k = d alpha/d p_k <g,x> + d beta/d p_k <g,y>
// (scalar results: g ds/dp_k in place of L_k, no alpha g / beta g term): ONE WAVE PER ROW, four rows per 256-thread block, as the forward
// kernel.  Pass 1 forms the five dot products in one sweep (float64 accumulators, wavefront xor-shuffles), the per-row scalar stage runs
// redundantly on all lanes, pass 2 writes gx and gy with coalesced stores.  No atomics, no LDS, no workspace; only x, y, g are read.
// The _c entry points read the curvature from one float on the device and give it a gradient: the scalar stage is
// evaluated a second time with c the one variable, each row's share of dL/dc goes to a float64 workspace and one workgroup adds them.
//
// The scalar stage is float64 forward-mode arithmetic (dual.hpp, struct DN<N>: a value and N partials; D3: the three partials d/dp_k): 1 - c |x|^2, 1 - u^2 under artanh
// and the Moebius denominator cancel near the ball boundary (pmath.hip's pair kernel and OP_PMEAN_PREP use float64 for the same reason).
// The stage is a few hundred float64 operations per row, tanh / log1p / sqrt among them, redundantly on 64 lanes (dist_matrix: once per
// pair); it is EXPECTED to stay below the row's memory traffic, and has not been timed.
// The primitives carry the derivative that the reference's autograd gives, not the textbook one:
//   * norm: 0 at a zero row (torch's subgradient), so a zero row of expmap0 / logmap0 gets g times the constant factor;
//   * clamp_min(1e-5) / tanh's clamp at 15: the gradient passes where the argument is inside (bounds included), else 0;
//   * artanh: value at the clamped argument, derivative 1 / (1 - x_clamped^2) (Artanh.backward, pmath.py:25-27) -- NOT zero outside the clamp;
//   * project: the clipped branch gets the gradient of maxnorm x / |x|; the branch is chosen by the forward kernel's own fp32 test;
//   * the + 1e-5 of the Moebius denominator.
// _hyperbolic_softmax's backward (per-pair coefficients, then row sums) and the feature clip of ToPoincare follow the same rules; their
// forms are described where they stand below.
#include "api_util.hpp"
#include "dual.hpp"
#include "pmath_curv.hpp"
#include "train_group.hpp"
#include <cmath>

extern "C" int sttode_tlinear(const float* X, long ldx, int xdiv, const float* W, long ldw, int trans, const float* bias, const float* mask,
                              long ldm, float* Y, long ldy, int cols, int J, int I, int act, int accumulate, void* stream);
extern "C" int sttode_twgrad(const float* dY, long ldy, const float* X, long ldx, int xdiv, float* dW, long ldw, float* db, int cols, int N,
                             int K, float* scratch, long scratch_floats, void* stream);
extern "C" int sttode_twgrad_flush(void);

namespace {

enum { OPB_PROJECT = 0, OPB_LAMBDA_X, OPB_MOBIUS_ADD, OPB_DIST, OPB_DIST0, OPB_EXPMAP, OPB_EXPMAP0, OPB_LOGMAP, OPB_LOGMAP0, OPB_P2K, OPB_K2P,
       OPB_LORENZ, OPB_COUNT };   // == the first twelve codes of pmath.hip's PmathOp (include/sttode_hip.h)

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wsumf(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The curvature in the scalar stage is a type CT: a plain double in the float-c entry points (no partial is carried for it, the
// arithmetic is the one this file always had), or one more forward-mode variable DN<N> in the _c entry points, where
// sqrt(c) is derived from it.  Every formula below is written once for both.
__device__ __forceinline__ double csqrt(double c) { return sqrt(c); }
template <int N> __device__ __forceinline__ DN<N> csqrt(const DN<N>& c) { return sqrt_(c); }

// _mobius_add(a, b) = (ca a + cb b) / den from the row scalars of its operands (pmath.py:171-177)
template <int N> struct MobD { DN<N> ca, cb; };
template <int N, class CT> __device__ __forceinline__ MobD<N> mob_d(const DN<N>& a2, const DN<N>& b2, const DN<N>& ab, const CT& c) {
    const DN<N> den = 1.0 + 2.0 * c * ab + (c * c) * (a2 * b2) + cst<N>(EPS5);
    return MobD<N>{(1.0 + 2.0 * c * ab + c * b2) / den, (1.0 - c * a2) / den};
}
// (-x) (+) y = A (-x) + B y and its norm (pmath.py:207, :335-336)
template <int N> struct SubD { DN<N> A, B, sn; };
template <int N, class CT> __device__ __forceinline__ SubD<N> sub_d(const DN<N>& p1, const DN<N>& p2, const DN<N>& p3, const CT& c) {
    const MobD<N> m = mob_d(p1, p2, -1.0 * p3, c);
    return SubD<N>{m.ca, m.cb, norm_of(m.ca * m.ca * p1 - 2.0 * (m.ca * m.cb * p3) + m.cb * m.cb * p2)};
}
// dist(x, y) (pmath.py:205-208) as a function of p = (|x|^2, |y|^2, <x,y>) and c
template <int N, class CT> __device__ __forceinline__ DN<N> dist_dn(const DN<N>& p1, const DN<N>& p2, const DN<N>& p3, const CT& c) {
    const CT sc = csqrt(c);
    const SubD<N> s = sub_d(p1, p2, p3, c);
    return (2.0 / sc) * artanh_d(sc * s.sn);
}
// ... its partials d/dp_k at a constant c (the tensor gradients), and its partial d/dc alone (the three scalars constants)
__device__ __forceinline__ D3 dist_d(double x2, double y2, double xy, double c) {
    return dist_dn(var<3>(x2, 0), var<3>(y2, 1), var<3>(xy, 2), c);
}
__device__ __forceinline__ double dist_dc(double x2, double y2, double xy, double c) {
    return dist_dn(cst<1>(x2), cst<1>(y2), cst<1>(xy), var<1>(c, 0)).d[0];
}

// ---- row ops --------------------------------------------------------------------------------------------------------------------------
// The scalar stage of the twelve row ops: alpha and beta (vector results) or al = s (scalar results) as functions of the row scalars p and
// the curvature.  Written once, evaluated in two forms: <3, double> -- p the variables, c a constant: the tensor gradients, the arithmetic
// this file always had -- and <1, DN<1>> -- c the variable, p constants: d/dc alone.  x2f, cf: the fp32 sum of squares and
// curvature of the forward kernel's own test, which chooses project's branch.
template <int N, class CT>
__device__ __forceinline__ void row_stage(int op, const DN<N>& p1, const DN<N>& p2, const DN<N>& p3, const CT& c, float x2f, float cf, DN<N>& al,
                                          DN<N>& be) {
    using D = DN<N>;
    const CT sc = csqrt(c);
    al = cst<N>(0.); be = cst<N>(0.);
    switch (op) {
        case OPB_PROJECT: {  // pmath.py:98-103 (maxnorm = (1 - 1e-3) / sqrt_c: the clipped branch depends on c)
            const float normf = fmaxf(sqrtf(x2f), 1e-5f), maxnormf = (1.0f - 1e-3f) / sqrtf(cf);
            const D norm = clamp_min_(norm_of(p1), EPS5);
            al = normf > maxnormf ? ((1.0 - 1e-3) / sc) / norm : cst<N>(1.0);
        } break;
        case OPB_LAMBDA_X: al = 2.0 / (1.0 - c * p1); break;   // pmath.py:128-129
        case OPB_MOBIUS_ADD: { const MobD<N> m = mob_d(p1, p2, p3, c); al = m.ca; be = m.cb; } break;
        case OPB_DIST: al = dist_dn(p1, p2, p3, c); break;
        case OPB_LOGMAP: {   // pmath.py:334-339 : 2 / sqrt_c / lambda_x * artanh(sqrt_c |sub|) * sub / |sub|
            const SubD<N> s = sub_d(p1, p2, p3, c);
            const D k = (1.0 - c * p1) / sc * artanh_d(sc * s.sn) / s.sn;
            al = -1.0 * (k * s.A); be = k * s.B;
        } break;
        case OPB_DIST0: al = (2.0 / sc) * artanh_d(sc * norm_of(p1)); break;   // pmath.py:231-234
        case OPB_EXPMAP: {   // pmath.py:268-277, y = u
            const D un = clamp_min_(norm_of(p2), EPS5);
            const D lam = 2.0 / (1.0 - c * p1);
            const D s = tanh_clamped_((sc / 2.0) * lam * un) / (sc * un);   // second_term = s u
            const MobD<N> m = mob_d(p1, s * s * p2, s * p3, c);
            al = m.ca; be = m.cb * s;
        } break;
        case OPB_EXPMAP0: {  // pmath.py:300-304
            const D un = clamp_min_(norm_of(p1), EPS5);
            al = tanh_clamped_(sc * un) / (sc * un);
        } break;
        case OPB_LOGMAP0: {  // pmath.py:365-368
            const D yn = clamp_min_(norm_of(p1), EPS5);
            al = 1.0 / yn / sc * artanh_d(sc * yn);
        } break;
        case OPB_P2K: al = 2.0 / (1.0 + c * p1); break;                  // pmath.py:440-442
        case OPB_K2P: al = 1.0 / (1.0 + sqrt_(1.0 - c * p1)); break;     // pmath.py:445-447
        case OPB_LORENZ: al = 1.0 / sqrt_(1.0 - c * p1); break;          // pmath.py:450-469
    }
}

// CG = false: the float-c form.  CG = true (the _c entry point): the curvature is read from cp[0]; after the float form's own stage, a
// second evaluation with c the one variable gives the row's share of dL/dc -- d alpha/dc <g,x> + d beta/dc <g,y>, or g ds/dc for a scalar
// result -- written to gc_ws[r] as one float64.  gx / gy may then be NULL (c alone requires a gradient): the second pass is skipped.
template <bool CG>
__global__ __launch_bounds__(256) void pmath_row_bwd_kernel(int op, const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ g, float* __restrict__ gx, float* __restrict__ gy,
                                                            int rows, int d, float cv, const float* __restrict__ cp,
                                                            double* __restrict__ gc_ws) {
    float cf = cv;
    if constexpr (CG) cf = *cp;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const bool scalar = op == OPB_LAMBDA_X || op == OPB_DIST || op == OPB_DIST0 || op == OPB_LORENZ;
    const float* xr = x + (size_t)r * d;
    const float* yr = y ? y + (size_t)r * d : nullptr;
    const float* gr = scalar ? nullptr : g + (size_t)r * d;
    double x2 = 0., y2 = 0., xy = 0., gxd = 0., gyd = 0.;
    float x2f = 0.f;   // project's branch: the forward kernel's own fp32 sum, same order
    for (int i = lane; i < d; i += 64) {
        const float af = xr[i];
        const double a = af, gi = gr ? (double)gr[i] : 0.;
        x2f += af * af;
        x2 += a * a; gxd += gi * a;
        if (yr) { const double b = yr[i]; y2 += b * b; xy += a * b; gyd += gi * b; }
    }
    x2 = wsum(x2); y2 = wsum(y2); xy = wsum(xy); gxd = wsum(gxd); gyd = wsum(gyd); x2f = wsumf(x2f);
    const double c = cf;
    if constexpr (CG) {
        DN<1> alc, bec;
        row_stage(op, cst<1>(x2), cst<1>(y2), cst<1>(xy), var<1>(c, 0), x2f, cf, alc, bec);
        if (lane == 0) gc_ws[r] = scalar ? (double)g[r] * alc.d[0] : alc.d[0] * gxd + bec.d[0] * gyd;
        if (!gx && !gy) return;
    }
    D3 al, be;   // vector results: alpha, beta; scalar results: al = s
    row_stage(op, var<3>(x2, 0), var<3>(y2, 1), var<3>(xy, 2), c, x2f, cf, al, be);
    // gx = ag g + ax x + ay y ; gy = bg g + by y + bx x
    double ag, ax, ay, bg, by, bx;
    if (scalar) {
        const double gs = g[r];
        ag = 0.; ax = 2.0 * gs * al.d[0]; ay = gs * al.d[2];
        bg = 0.; by = 2.0 * gs * al.d[1]; bx = ay;
    } else {
        const double L1 = al.d[0] * gxd + be.d[0] * gyd, L2 = al.d[1] * gxd + be.d[1] * gyd, L3 = al.d[2] * gxd + be.d[2] * gyd;
        ag = al.v; ax = 2.0 * L1; ay = L3;
        bg = be.v; by = 2.0 * L2; bx = L3;
    }
    float* gxr = (!CG || gx) ? gx + (size_t)r * d : nullptr;
    float* gyr = yr && (!CG || gy) ? gy + (size_t)r * d : nullptr;
    for (int i = lane; i < d; i += 64) {
        const double a = xr[i], b = yr ? (double)yr[i] : 0., gi = gr ? (double)gr[i] : 0.;
        if (!CG || gxr) gxr[i] = (float)(ag * gi + ax * a + ay * b);
        if (gyr) gyr[i] = (float)(bg * gi + by * b + bx * a);
    }
}

// ---- mobius_matvec (pmath.py:399-408) back through _project, the tanh(|mx| / |x| artanh(sqrt_c |x|)) mx / (|mx| sqrt_c) factor and the
// mx == 0 branch: out = alpha(q) mx with q = (|mx|^2, |x|).  One wave per row: gmx = alpha g + 2 mx d alpha/d q1 <g,mx>, and
// gxn = dL/d|x| = d alpha/d q2 <g,mx>; the row of gx is started as gxn x / |x| (0 at a zero row), the GEMM adds gmx m to it.  gxn is also
// written to gxn_ws, an output nothing here reads.
// _project's branch is chosen here by a float64 test on the recomputed mx; the forward kernel (pmath.hip OP_MATVEC_FIN) chose it with fp32
// norms of ITS mx (a sequential fp32 dot product, where this one comes from the training GEMM), so its test cannot be repeated bit for
// bit: a row whose |res| is within fp32 rounding of maxnorm may get the gradient of the other branch than its forward value came from.
// The scalar stage, alpha(|mx|^2, |x|, c), once for both forms as row_stage is: <3, double> with q the variables (slots 0, 1), and
// <1, DN<1>> with c the variable.  CG = true (the _c entry point): c is read from cp[0]; d alpha/dc <g,mx> -- through alpha's own sqrt_c
// and through _project's maxnorm; mx does not depend on c -- goes to gc_ws[r]; gmx, gxn and gx may be NULL (nothing needs them).
__device__ __forceinline__ double val_of(double a) { return a; }
template <int N> __device__ __forceinline__ double val_of(const DN<N>& a) { return a.v; }
template <int N, class CT> __device__ __forceinline__ DN<N> matvec_stage(const DN<N>& q1, const DN<N>& xnq, const CT& c) {
    using D = DN<N>;
    const CT sc = csqrt(c);
    const D xn = clamp_min_(xnq, EPS5);
    const D mxn = norm_of(q1);
    const D ga = tanh_clamped_(mxn / xn * artanh_d(sc * xn)) / (mxn * sc);   // res = ga mx
    const D norm = clamp_min_(norm_of(ga * ga * q1), EPS5);                 // _project, pmath.py:98-103
    const CT maxnorm = (1.0 - 1e-3) / sc;
    return norm.v > val_of(maxnorm) ? ga * (maxnorm / norm) : ga;
}
template <bool CG>
__global__ __launch_bounds__(256) void pmath_matvec_bwd_kernel(const float* __restrict__ mx, const float* __restrict__ x, const float* __restrict__ g,
                                                               float* __restrict__ gmx, float* __restrict__ gxn, float* __restrict__ gx, int rows,
                                                               int d, int O, float cv, const float* __restrict__ cp,
                                                               double* __restrict__ gc_ws) {
    float cf = cv;
    if constexpr (CG) cf = *cp;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* mr = mx + (size_t)r * O;
    const float* gr = g + (size_t)r * O;
    const float* xr = x + (size_t)r * d;
    double m2 = 0., gm = 0., x2 = 0.;
    for (int i = lane; i < O; i += 64) { const double a = mr[i]; m2 += a * a; gm += (double)gr[i] * a; }
    for (int i = lane; i < d; i += 64) { const double a = xr[i]; x2 += a * a; }
    m2 = wsum(m2); gm = wsum(gm); x2 = wsum(x2);
    const double c = cf, xnv = sqrt(x2);
    if constexpr (CG) {
        if (lane == 0) gc_ws[r] = m2 > 0. ? matvec_stage(cst<1>(m2), cst<1>(xnv), var<1>(c, 0)).d[0] * gm : 0.;
        if (!gmx && !gx) return;
    }
    double a0 = 0., c1 = 0., dn = 0.;   // mx == 0: zero gradient (the reference's 0/0 behind torch.where gives NaN)
    if (m2 > 0.) {
        const D3 al = matvec_stage(var<3>(m2, 0), var<3>(xnv, 1), c);
        a0 = al.v; c1 = 2.0 * al.d[0] * gm; dn = al.d[1] * gm;
    }
    if (!CG || gmx) {
        float* go = gmx + (size_t)r * O;
        for (int i = lane; i < O; i += 64) go[i] = (float)(a0 * (double)gr[i] + c1 * (double)mr[i]);
    }
    if (lane == 0 && (!CG || gxn)) gxn[r] = (float)dn;
    if (CG && !gx) return;
    const double kx = xnv > 0. ? dn / xnv : 0.;
    float* gxr = gx + (size_t)r * d;
    for (int i = lane; i < d; i += 64) gxr[i] = (float)(kx * (double)xr[i]);
}

// ---- dist_matrix (pmath.py:482-493): out[p, q] = dist(x_p, y_q).  side 0: one wave per x row sums g[p, q] (2 x_p ds/dp1 + y_q ds/dp3) over
// its R partners -> gx; side 1: one wave per y row sums g[p, q] (2 y_q ds/dp2 + x_p ds/dp3) over its P partners -> gy.  Partners in index
// order, every sum in a fixed order: bitwise repeatable, no atomics.  Scalars in float64 as in the forward pair kernel.  Each lane keeps
// four elements of the row's sum; a row longer than 256 takes one sweep over the partners per 256 elements.
// CPTR: the curvature is read from cp[0] (the _c entry point), the arithmetic of the tensor gradients unchanged.  CG (side 0 of the _c
// entry point only): the row's sum over its partners, in index order, of g[p, q] ds/dc -- dist_dc, a second evaluation with c the one
// variable -- goes to gc_ws[r] (taken in the first 256-element sweep); gout may then be NULL.
template <bool CG, bool CPTR>
__global__ __launch_bounds__(256) void pmath_dist_matrix_bwd_kernel(int side, const float* __restrict__ x, const float* __restrict__ y,
                                                                    const float* __restrict__ g, float* __restrict__ gout, int P, int R, int d,
                                                                    float cv, const float* __restrict__ cp, double* __restrict__ gc_ws) {
    float cf = cv;
    if constexpr (CPTR) cf = *cp;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_self = side ? R : P, n_part = side ? P : R;
    if (r >= n_self) return;
    const float* self = (side ? y : x) + (size_t)r * d;
    const float* part = side ? x : y;
    const double c = cf;
    double s2 = 0.;
    for (int i = lane; i < d; i += 64) { const double a = self[i]; s2 += a * a; }
    s2 = wsum(s2);
    for (int base = 0; base < d; base += 256) {
        double acc[4] = {0., 0., 0., 0.}, ks = 0., kc = 0.;
        for (int q = 0; q < n_part; ++q) {
            const float* pr = part + (size_t)q * d;
            double q2 = 0., sq = 0.;
            for (int i = lane; i < d; i += 64) { const double a = self[i], b = pr[i]; q2 += b * b; sq += a * b; }
            q2 = wsum(q2); sq = wsum(sq);
            if constexpr (CG) {
                if (base == 0)
                    kc += (double)(side ? g[(size_t)q * R + r] : g[(size_t)r * R + q]) * (side ? dist_dc(q2, s2, sq, c) : dist_dc(s2, q2, sq, c));
                if (!gout) continue;
            }
            const D3 s = side ? dist_d(q2, s2, sq, c) : dist_d(s2, q2, sq, c);
            const double gv = side ? g[(size_t)q * R + r] : g[(size_t)r * R + q];
            ks += 2.0 * gv * s.d[side ? 1 : 0];
            const double kp = gv * s.d[2];
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int i = base + lane + 64 * j; if (i < d) acc[j] += kp * (double)pr[i]; }
        }
        if constexpr (CG) {
            if (base == 0 && lane == 0) gc_ws[r] = kc;
            if (!gout) return;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int i = base + lane + 64 * j; if (i < d) gout[(size_t)r * d + i] = (float)(ks * (double)self[i] + acc[j]); }
    }
}

// ---- _hyperbolic_softmax (pmath.py:430-437): logit[q, p] is a function of six scalars of the pair, z = (|P_p|^2, |X_q|^2, <P_p,X_q>,
// |A_p|^2, <A_p,P_p>, <A_p,X_q>): with ca = 1 - 2c z2 + c z1, cb = 1 - c z0, den = 1 - 2c z2 + c^2 z0 z1 + 1e-5 the Moebius sum v = (-P) (+) X
// has <v,A> = (cb z5 - ca z4) / den and |v|^2 = (ca^2 z0 - 2 ca cb z2 + cb^2 z1) / den^2, and
//     logit = 2 / cb * sqrt(z3) / sqrt_c * arsinh(2 sqrt_c <v,A> / (sqrt(z3) (1 - c |v|^2))).
// Every input gradient is then a sum of rows weighted by w_k[q, p] = g[q, p] d logit / d z_k:
//     gX_q = 2 X_q sum_p w1 + sum_p w2 P_p + sum_p w5 A_p
//     gP_p = 2 P_p sum_q w0 + A_p sum_q w4 + sum_q w2 X_q          gA_p = 2 A_p sum_q w3 + P_p sum_q w4 + sum_q w5 X_q
// The coefficient kernel (one wave per pair) forms the six scalars in float64 -- as the forward pair kernel does, for the same cancellation in
// cb and 1 - c |v|^2 -- and writes w [6,B,C] once per pair; the row-sum kernel (one wave per output row, partners in index order, each lane
// four elements of the row, one sweep over the partners per 256 elements) adds the rows: no atomics, every sum in a fixed order.
template <int N, class CT>
__device__ __forceinline__ DN<N> hsoftmax_dn(const DN<N>& p, const DN<N>& x, const DN<N>& t, const DN<N>& a, const DN<N>& b, const DN<N>& g,
                                            const CT& c) {
    const CT sc = csqrt(c);
    const DN<N> ca = 1.0 - 2.0 * c * t + c * x, cb = 1.0 - c * p;
    const DN<N> den = 1.0 - 2.0 * c * t + (c * c) * (p * x) + cst<N>(EPS5);
    const DN<N> va = (cb * g - ca * b) / den;
    const DN<N> v2 = (ca * ca * p - 2.0 * (ca * cb * t) + cb * cb * x) / (den * den);
    const DN<N> an = norm_of(a);
    return (2.0 / sc) * an / cb * arsinh_d((2.0 * sc) * va / (an * (1.0 - c * v2)));
}
__device__ __forceinline__ D6 hsoftmax_d(double pi, double xi, double tau, double al, double be, double ga, double c) {
    return hsoftmax_dn(var<6>(pi, 0), var<6>(xi, 1), var<6>(tau, 2), var<6>(al, 3), var<6>(be, 4), var<6>(ga, 5), c);
}

// CG = true (the _c entry point): c is read from cp[0]; after the float form's six partials, a second evaluation with c the one variable
// gives the seventh plane of w, g[b, k] d logit / dc.
template <bool CG>
__global__ __launch_bounds__(256) void pmath_hsoftmax_coef_kernel(const float* __restrict__ X, const float* __restrict__ A, const float* __restrict__ P,
                                                                  const float* __restrict__ g, double* __restrict__ w, int B, int C, int d,
                                                                  float cv, const float* __restrict__ cp) {
    float cf = cv;
    if constexpr (CG) cf = *cp;
    const int lane = threadIdx.x & 63;
    const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6), BC = (long)B * C;
    if (pair >= BC) return;
    const float* xr = X + (size_t)(pair / C) * d;
    const float* ar = A + (size_t)(pair % C) * d;
    const float* pr = P + (size_t)(pair % C) * d;
    double pi = 0., xi = 0., tau = 0., al = 0., be = 0., ga = 0.;
    for (int i = lane; i < d; i += 64) {
        const double pv = pr[i], xv = xr[i], av = ar[i];
        pi += pv * pv; xi += xv * xv; tau += pv * xv; al += av * av; be += av * pv; ga += av * xv;
    }
    pi = wsum(pi); xi = wsum(xi); tau = wsum(tau); al = wsum(al); be = wsum(be); ga = wsum(ga);
    const D6 L = hsoftmax_d(pi, xi, tau, al, be, ga, (double)cf);
    if (lane == 0) {
        const double gv = g[pair];
#pragma unroll
        for (int k = 0; k < 6; ++k) w[(size_t)k * BC + pair] = gv * L.d[k];
        if constexpr (CG)
            w[(size_t)6 * BC + pair] = gv * hsoftmax_dn(cst<1>(pi), cst<1>(xi), cst<1>(tau), cst<1>(al), cst<1>(be), cst<1>(ga), var<1>((double)cf, 0)).d[0];
    }
}

// side 0: one wave per X row -> gX; side 1: one wave per class row -> gP and gA (both sum the same partners, the X rows)
// CG = true (the _c entry point, side 0 only): the row's sum of the seventh plane over its classes, in index order, goes to gc_ws[r];
// gX may be NULL.
template <bool CG>
__global__ __launch_bounds__(256) void pmath_hsoftmax_rowsum_kernel(int side, const float* __restrict__ X, const float* __restrict__ A,
                                                                    const float* __restrict__ P, const double* __restrict__ w,
                                                                    float* __restrict__ gX, float* __restrict__ gA, float* __restrict__ gP, int B,
                                                                    int C, int d, double* __restrict__ gc_ws) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_self = side ? C : B, n_part = side ? B : C;
    if (r >= n_self) return;
    const size_t BC = (size_t)B * C;
    const float* trow = side ? X : P;   // the partner rows that w2 weights
    const float* grow = side ? X : A;   // ... and w5
    if constexpr (CG) {
        double kc = 0.;
        for (int j = 0; j < n_part; ++j) kc += w[6 * BC + (size_t)r * C + j];
        if (lane == 0) gc_ws[r] = kc;
        if (!gX) return;
    }
    for (int base = 0; base < d; base += 256) {
        double at[4] = {0., 0., 0., 0.}, ag[4] = {0., 0., 0., 0.}, s0 = 0., s3 = 0., s4 = 0.;
        for (int j = 0; j < n_part; ++j) {
            const size_t pair = side ? (size_t)j * C + r : (size_t)r * C + j;
            const double wt = w[2 * BC + pair], wg = w[5 * BC + pair];
            if (side) { s0 += w[pair]; s3 += w[3 * BC + pair]; s4 += w[4 * BC + pair]; }
            else s0 += w[BC + pair];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = base + lane + 64 * k;
                if (i < d) { at[k] += wt * (double)trow[(size_t)j * d + i]; ag[k] += wg * (double)grow[(size_t)j * d + i]; }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = base + lane + 64 * k;
            if (i >= d) continue;
            const size_t o = (size_t)r * d + i;
            if (side) {
                const double pv = P[o], av = A[o];
                gP[o] = (float)(2.0 * s0 * pv + s4 * av + at[k]);
                gA[o] = (float)(2.0 * s3 * av + s4 * pv + ag[k]);
            } else {
                gX[o] = (float)(2.0 * s0 * (double)X[o] + at[k] + ag[k]);
            }
        }
    }
}

// ---- feature clipping (hyptorch/nn.py:154-160, ToPoincare(clip_r=r)): out = x min(1, r / (|x| + 1e-5)).  One wave per row, the norm in
// float64.  Backward: an unclipped row passes g; a clipped one gets s g - x <g,x> s / ((|x| + 1e-5) |x|) with s = r / (|x| + 1e-5).
__global__ __launch_bounds__(256) void pmath_clip_kernel(const float* __restrict__ x, float* __restrict__ out, int rows, int d, float rf) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* xr = x + (size_t)r * d;
    double x2 = 0.;
    for (int i = lane; i < d; i += 64) { const double a = xr[i]; x2 += a * a; }
    const double s = fmin(1.0, (double)rf / (sqrt(wsum(x2)) + EPS5));
    for (int i = lane; i < d; i += 64) out[(size_t)r * d + i] = (float)(s * (double)xr[i]);
}

__global__ __launch_bounds__(256) void pmath_clip_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ gx,
                                                             int rows, int d, float rf) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* xr = x + (size_t)r * d;
    const float* gr = g + (size_t)r * d;
    double x2 = 0., gxd = 0.;
    for (int i = lane; i < d; i += 64) { const double a = xr[i]; x2 += a * a; gxd += (double)gr[i] * a; }
    x2 = wsum(x2); gxd = wsum(gxd);
    const double n = sqrt(x2), s = (double)rf / (n + EPS5);
    const bool clipped = s < 1.0;   // (then n > r - 1e-5 > 0 is not guaranteed for r <= 1e-5: a zero row is never divided by)
    const double kg = clipped ? s : 1.0, kx = clipped && n > 0. ? -gxd * s / ((n + EPS5) * n) : 0.;
    for (int i = lane; i < d; i += 64) gx[(size_t)r * d + i] = (float)(kg * (double)gr[i] + kx * (double)xr[i]);
}

// ---- dL/dc: the per-row float64 shares of gc_ws[rows] -> gc[0].  ONE workgroup of 256 threads: thread t sums rows t, t + 256, ... in
// that order, then a fixed LDS tree (stride 128, 64, ..., 1) adds the 256 partial sums.  No atomics; the order depends on rows alone, so
// the float that is stored -- written, not accumulated -- is bitwise repeatable.
__global__ __launch_bounds__(256) void pmath_gc_finish_kernel(const double* __restrict__ gc_ws, float* __restrict__ gc, long rows) {
    __shared__ double part[256];
    double s = 0.;
    for (long i = threadIdx.x; i < rows; i += 256) s += gc_ws[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) gc[0] = (float)part[0];
}

// ---- poincare_mean (pmath.py:472-479) over the middle dimension of x [outer, R, inner, d].  With q_r = 1 - c |x_r|^2,
// S = sum_r 2 x_r / q_r, L = sum_r (1 + c |x_r|^2) / q_r, m = S / L (the Klein mean) and y = k2p(m) = al(p) m, p = |m|^2,
// al = 1 / (1 + s), s = sqrt(1 - c p):
//     g_m = al g + 2 al' <g,m> m,  al' = c / (2 s (1 + s)^2);   g_S = g_m / L;   g_L = -<g_m,m> / L;
//     gx_r = (2 / q_r) g_S + (4 c / q_r^2) (<x_r,g_S> + g_L) x_r.
// TWO launches.  The group stage, one wave per group (o, n): S and L are RECOMPUTED in float64 from x (the forward's fp32 sums are not
// used), rows in index order, each lane four elements of S per 256-element sweep; S goes to gS_ws, the dot products |S|^2 and <g,S> close
// the scalars, and the lane that wrote an element of S overwrites it with g_S; g_L goes to gL_ws.  The row stage, one wave per row: |x_r|^2
// and <x_r,g_S> in one sweep, gx in the second.  dL/dc (CG): a row's share is (2 |x_r|^2 / q_r^2) (<x_r,g_S> + g_L) -- through
// d(2 x / q)/dc and d lambda/dc -- to gc_ws[row]; a group's share through k2p is <g,m> p / (2 s (1 + s)^2), to gc_ws[rows + group].
template <bool CPTR, bool CG>
__global__ __launch_bounds__(256) void pmath_mean_group_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, double* __restrict__ gS,
                                                                   double* __restrict__ gL, int groups, int R, int inner, int d, float cv,
                                                                   const float* __restrict__ cp, double* __restrict__ gc_groups) {
    float cf = cv;
    if constexpr (CPTR) cf = *cp;
    const int lane = threadIdx.x & 63;
    const int grp = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (grp >= groups) return;
    const double c = cf;
    const size_t o = grp / inner, n = grp % inner, rs = (size_t)inner * d;
    const float* x0 = x + (o * R * inner + n) * d;      // row r of the group: x0 + r rs
    const float* gr = g + (size_t)grp * d;
    double* Sr = gS + (size_t)grp * d;
    double L = 0., SS = 0., GS = 0.;
    for (int base = 0; base < d; base += 256) {
        double acc[4] = {0., 0., 0., 0.};
        for (int r = 0; r < R; ++r) {
            const float* xr = x0 + (size_t)r * rs;
            double x2 = 0.;
            for (int i = lane; i < d; i += 64) { const double a = xr[i]; x2 += a * a; }
            x2 = wsum(x2);
            const double q = 1.0 - c * x2;
            if (base == 0) L += (1.0 + c * x2) / q;
            const double k = 2.0 / q;
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int i = base + lane + 64 * j; if (i < d) acc[j] += k * (double)xr[i]; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = base + lane + 64 * j;
            if (i < d) { Sr[i] = acc[j]; SS += acc[j] * acc[j]; GS += (double)gr[i] * acc[j]; }
        }
    }
    SS = wsum(SS); GS = wsum(GS);
    const double p = SS / (L * L), gm = GS / L;                     // |m|^2, <g,m>
    const double s = sqrt(1.0 - c * p), al = 1.0 / (1.0 + s), dal = c / (2.0 * s * (1.0 + s) * (1.0 + s));
    const double kS = 2.0 * dal * gm / L;                            // g_m = al g + kS S
    for (int i = lane; i < d; i += 64) Sr[i] = (al * (double)gr[i] + kS * Sr[i]) / L;
    if (lane == 0) {
        gL[grp] = -(al * gm + 2.0 * dal * gm * p) / L;
        if constexpr (CG) gc_groups[grp] = gm * p / (2.0 * s * (1.0 + s) * (1.0 + s));
    }
}

template <bool CPTR, bool CG>
__global__ __launch_bounds__(256) void pmath_mean_row_bwd_kernel(const float* __restrict__ x, const double* __restrict__ gS,
                                                                 const double* __restrict__ gL, float* __restrict__ gx, int rows, int R, int inner,
                                                                 int d, float cv, const float* __restrict__ cp, double* __restrict__ gc_ws) {
    float cf = cv;
    if constexpr (CPTR) cf = *cp;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const double c = cf;
    const size_t grp = (size_t)(r / (R * inner)) * inner + r % inner;
    const float* xr = x + (size_t)r * d;
    const double* Sr = gS + grp * d;
    double x2 = 0., xs = 0.;
    for (int i = lane; i < d; i += 64) { const double a = xr[i]; x2 += a * a; xs += a * Sr[i]; }
    x2 = wsum(x2); xs = wsum(xs);
    const double q = 1.0 - c * x2, t = (xs + gL[grp]) / (q * q);
    if constexpr (CG) {
        if (lane == 0) gc_ws[r] = 2.0 * x2 * t;
        if (!gx) return;
    }
    const double k1 = 2.0 / q, k2 = 4.0 * c * t;
    for (int i = lane; i < d; i += 64) gx[(size_t)r * d + i] = (float)(k1 * Sr[i] + k2 * (double)xr[i]);
}

// ---- Oblique.proj (core/manifolds/oblique.py:15-16), y = p / |p|: gp = (g - <g,y> y) / |p|.  A zero row gives NaN, as the forward does.
__global__ __launch_bounds__(256) void oblique_proj_bwd_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ gp,
                                                               int rows, int d) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* pr = p + (size_t)r * d;
    const float* gr = g + (size_t)r * d;
    double p2 = 0., gpd = 0.;
    for (int i = lane; i < d; i += 64) { const double a = pr[i]; p2 += a * a; gpd += (double)gr[i] * a; }
    p2 = wsum(p2); gpd = wsum(gpd);
    const double n = sqrt(p2), kg = 1.0 / n, kp = -gpd / (p2 * n);
    for (int i = lane; i < d; i += 64) gp[(size_t)r * d + i] = (float)(kg * (double)gr[i] + kp * (double)pr[i]);
}

// ---- Oblique.dist (oblique.py:36-43): out[b, i, j] = acos(clamp(<p2_i, p1_j>, +-(1 - 1e-4))).  coef_ij = -g_ij / sqrt(1 - s_ij^2) where the
// un-clamped inner product s_ij lies within the clamp (bounds included: torch.clamp's gradient), else 0; gp2_i = sum_j coef_ij p1_j (side
// 0, one wave per p2 row), gp1_j = sum_i coef_ij p2_i (side 1, one wave per p1 row).  Partners in index order, the inner product in float64,
// each lane four elements of the row per 256-element sweep, as pmath_dist_matrix_bwd_kernel; nb batches.
__global__ __launch_bounds__(256) void oblique_dist_bwd_kernel(int side, const float* __restrict__ p1, const float* __restrict__ p2,
                                                               const float* __restrict__ g, float* __restrict__ gout, int nb, int n1, int n2, int d) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_self = side ? n1 : n2, n_part = side ? n2 : n1;
    if (r >= (long)nb * n_self) return;
    const long bt = r / n_self, k = r % n_self;
    const float* self = (side ? p1 : p2) + (size_t)r * d;
    const float* part = (side ? p2 : p1) + (size_t)bt * n_part * d;
    const float* gb = g + (size_t)bt * n2 * n1;
    const double hi = (double)(1.0f - 1e-4f), lo = (double)(-1.0f + 1e-4f);
    for (int base = 0; base < d; base += 256) {
        double acc[4] = {0., 0., 0., 0.};
        for (int q = 0; q < n_part; ++q) {
            const float* pr = part + (size_t)q * d;
            double s = 0.;
            for (int i = lane; i < d; i += 64) s += (double)self[i] * (double)pr[i];
            s = wsum(s);
            const double gv = side ? gb[(size_t)q * n1 + k] : gb[(size_t)k * n1 + q];
            const double coef = (s >= lo && s <= hi) ? -gv / sqrt(1.0 - s * s) : 0.;
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int i = base + lane + 64 * j; if (i < d) acc[j] += coef * (double)pr[i]; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int i = base + lane + 64 * j; if (i < d) gout[(size_t)r * d + i] = (float)acc[j]; }
    }
}

}  // namespace

// poincare_mean backward: x [outer,R,inner,d], g [outer,inner,d] -> gx as x.  Workspaces gS_ws [outer inner d] and gL_ws [outer inner]
// doubles.  Two launches; bitwise repeatable, no atomics.  Device form: gc_ws holds outer R inner + outer inner doubles (the rows'
// shares, then the groups'), and gx may be NULL (c alone requires a gradient).
static int pmath_mean_bwd(const char* who, const float* x, const float* g, double* gS_ws, double* gL_ws, float* gx, int outer, int R, int inner,
                          int d, Curv cv, void* stream) {
    PM_REQUIRE_CURV();
    PM_REQUIRE(x && g && gS_ws && gL_ws && (cv.dev || gx), "null pointer");
    PM_REQUIRE(!cv.dev || (cv.gc_ws && cv.gc), "gc_ws [rows + groups] doubles and gc [1] are required");
    PM_REQUIRE(outer > 0 && R > 0 && inner > 0 && d > 0, "empty shape");
    PM_REQUIRE((long)outer * R * inner <= 0x7fffffffL, "more than 2^31 - 1 rows");
    PM_REQUIRE(cv.dev || (cv.c > 0.f && std::isfinite(cv.c)), "curvature c must be positive and finite");
    hipStream_t s = (hipStream_t)stream;
    const int groups = outer * inner, rows = groups * R;
    auto group = pmath_mean_group_bwd_kernel<true, true>;
    auto row = pmath_mean_row_bwd_kernel<true, true>;
    if (!cv.dev) group = pmath_mean_group_bwd_kernel<false, false>, row = pmath_mean_row_bwd_kernel<false, false>;
    hipLaunchKernelGGL(group, dim3((groups + 3) / 4), dim3(256), 0, s, x, g, gS_ws, gL_ws, groups, R, inner, d, cv.c, cv.c_dev,
                       cv.dev ? cv.gc_ws + rows : nullptr);
    hipLaunchKernelGGL(row, dim3((rows + 3) / 4), dim3(256), 0, s, x, (const double*)gS_ws, (const double*)gL_ws, gx, rows, R, inner, d, cv.c,
                       cv.c_dev, cv.gc_ws);
    if (cv.dev) hipLaunchKernelGGL(pmath_gc_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)cv.gc_ws, cv.gc, (long)rows + groups);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_pmath_mean_bwd(const float* x, const float* g, double* gS_ws, double* gL_ws, float* gx, int outer, int R, int inner, int d,
                                     float c, void* stream) {
    return pmath_mean_bwd("sttode_pmath_mean_bwd", x, g, gS_ws, gL_ws, gx, outer, R, inner, d, curv_float(c), stream);
}

extern "C" int sttode_pmath_mean_bwd_c(const float* x, const float* g, double* gS_ws, double* gL_ws, float* gx, int outer, int R, int inner,
                                       int d, const float* c_dev, double* gc_ws, float* gc, void* stream) {
    return pmath_mean_bwd("sttode_pmath_mean_bwd_c", x, g, gS_ws, gL_ws, gx, outer, R, inner, d, curv_dev(c_dev, gc_ws, gc), stream);
}

extern "C" int sttode_oblique_proj_bwd(const float* p, const float* g, float* gp, int rows, int d, void* stream) {
    STT_REQUIRE(p && g && gp, "sttode_oblique_proj_bwd: null pointer");
    STT_REQUIRE(rows > 0 && d > 0, "sttode_oblique_proj_bwd: empty shape");
    hipLaunchKernelGGL(oblique_proj_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, p, g, gp, rows, d);
    STT_HIP(hipGetLastError());
    return 0;
}

// Oblique.dist backward: p1 [nb,n1,d], p2 [nb,n2,d], g [nb,n2,n1] -> gp1, gp2 (each may be NULL; not both).  One launch per output.
extern "C" int sttode_oblique_dist_bwd(const float* p1, const float* p2, const float* g, float* gp1, float* gp2, int nb, int n1, int n2, int d,
                                       void* stream) {
    STT_REQUIRE(p1 && p2 && g && (gp1 || gp2), "sttode_oblique_dist_bwd: null pointer");
    STT_REQUIRE(nb > 0 && n1 > 0 && n2 > 0 && d > 0, "sttode_oblique_dist_bwd: empty shape");
    hipStream_t s = (hipStream_t)stream;
    if (gp2)
        hipLaunchKernelGGL(oblique_dist_bwd_kernel, dim3((unsigned)(((long)nb * n2 + 3) / 4)), dim3(256), 0, s, 0, p1, p2, g, gp2, nb, n1, n2, d);
    if (gp1)
        hipLaunchKernelGGL(oblique_dist_bwd_kernel, dim3((unsigned)(((long)nb * n1 + 3) / 4)), dim3(256), 0, s, 1, p1, p2, g, gp1, nb, n1, n2, d);
    STT_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// One host function per backward pass for its two exported forms (pmath_curv.hpp).  The float form requires every gradient buffer and
// checks c > 0; it launches the <false> instantiations and no finishing kernel.  The device form: the curvature is ONE
// float on the device, c_dev, and gets a gradient.  Each row kernel (<true>) writes its rows' float64 shares of dL/dc to gc_ws (one double
// per row of the op: rows, rows, P, B), pmath_gc_finish_kernel adds them in a fixed order and WRITES the float gc[0].  The tensor
// gradients may be NULL when nothing needs them; where they are given, their values are bitwise those of the float form at c = *c_dev.
// *c_dev cannot be checked here: a curvature that is not positive gives NaN, not a refusal.  (Where a function names both instantiations
// of a kernel, it names them in the order the device code has always been emitted in.)
static int pmath_rowop_bwd(const char* who, int op, const float* x, const float* y, const float* g, float* gx, float* gy, int rows, int d,
                           Curv cv, void* stream) {
    PM_REQUIRE_CURV();
    PM_REQUIRE(op != 12, "Oblique.proj has no backward pass here");
    PM_REQUIRE(op != 13 && op != 14, "the internal halves of mobius_matvec / poincare_mean have no backward pass here");
    PM_REQUIRE(op >= 0 && op < OPB_COUNT, "unknown op");
    PM_REQUIRE(x && g && (cv.dev || gx) && rows > 0 && d > 0, "null pointer or empty shape");
    PM_REQUIRE(!cv.dev || (cv.gc_ws && cv.gc), "gc_ws [rows] doubles and gc [1] are required");
    const bool needs_y = op == OPB_MOBIUS_ADD || op == OPB_DIST || op == OPB_LOGMAP || op == OPB_EXPMAP;
    if (cv.dev) PM_REQUIRE(!needs_y || y, "this op needs a second operand y");
    else PM_REQUIRE(!needs_y || (y && gy), "this op needs a second operand and its gradient buffer gy");
    PM_REQUIRE(needs_y || !gy, "gy given for an op with one operand");
    PM_REQUIRE(cv.dev || cv.c > 0.f, "curvature c must be positive");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(!cv.dev ? pmath_row_bwd_kernel<false> : pmath_row_bwd_kernel<true>, dim3((rows + 3) / 4), dim3(256), 0, s, op, x,
                       needs_y ? y : nullptr, g, gx, needs_y ? gy : nullptr, rows, d, cv.c, cv.c_dev, cv.gc_ws);
    if (cv.dev) hipLaunchKernelGGL(pmath_gc_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)cv.gc_ws, cv.gc, (long)rows);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_pmath_rowop_bwd(int op, const float* x, const float* y, const float* g, float* gx, float* gy, int rows, int d, float c,
                                      void* stream) {
    return pmath_rowop_bwd("sttode_pmath_rowop_bwd", op, x, y, g, gx, gy, rows, d, curv_float(c), stream);
}

extern "C" int sttode_pmath_rowop_bwd_c(int op, const float* x, const float* y, const float* g, float* gx, float* gy, int rows, int d,
                                        const float* c_dev, double* gc_ws, float* gc, void* stream) {
    return pmath_rowop_bwd("sttode_pmath_rowop_bwd_c", op, x, y, g, gx, gy, rows, d, curv_dev(c_dev, gc_ws, gc), stream);
}

// mobius_matvec backward.  mx = x m^T is recomputed into mx_ws by the training GEMM (the autograd function saves only m and x); after the
// row kernel has read it, mx_ws holds the split sums of the weight gradient.  gx = gmx m + gxn x / |x| (sttode_tlinear, trans = 1, adding to
// the rows the row kernel started); gm = gmx^T x (sttode_twgrad, which accumulates: gm is zeroed first).  gxn_ws [rows] receives dL/d|x|
// per row: an OUTPUT that no later launch reads (the row kernel puts that term into gx itself).
// Float form: no buffer may be NULL, gxn_ws included.  Device form: gx and gm may each be NULL (then its GEMM is not run); gmx_ws may be
// NULL when both are, gxn_ws always.
// DEVIATION from the reference: a row with mx == 0 (a zero x row) gets a zero gradient; the reference's 0/0 behind torch.where gives NaN.
static int pmath_matvec_bwd(const char* who, const float* m, const float* x, const float* g, float* mx_ws, float* gmx_ws, float* gxn_ws,
                            float* gx, float* gm, int rows, int d, int O, Curv cv, void* stream) {
    PM_REQUIRE_CURV();
    PM_REQUIRE(m && x && g && mx_ws && (cv.dev || (gmx_ws && gxn_ws && gx && gm)), "null pointer");
    PM_REQUIRE(gmx_ws || (!gx && !gm), "gx and gm need the workspace gmx_ws");
    PM_REQUIRE(!cv.dev || (cv.gc_ws && cv.gc), "gc_ws [rows] doubles and gc [1] are required");
    PM_REQUIRE(rows > 0 && d > 0 && O > 0, "rows, d, O must be positive");
    PM_REQUIRE(cv.dev || cv.c > 0.f, "curvature c must be positive");
    PM_REQUIRE(!stt_tgemm_group_open(), "not inside a sttode_tgemm_group bracket (its products depend on each other)");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = sttode_tlinear(x, d, 1, m, d, 0, nullptr, nullptr, 0, mx_ws, O, rows, d, O, 0, 0, stream)) return rc;
    hipLaunchKernelGGL(!cv.dev ? pmath_matvec_bwd_kernel<false> : pmath_matvec_bwd_kernel<true>, dim3((rows + 3) / 4), dim3(256), 0, s,
                       (const float*)mx_ws, x, g, gmx_ws, gxn_ws, gx, rows, d, O, cv.c, cv.c_dev, cv.gc_ws);
    if (cv.dev) hipLaunchKernelGGL(pmath_gc_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)cv.gc_ws, cv.gc, (long)rows);
    STT_HIP(hipGetLastError());
    if (gx)
        if (int rc = sttode_tlinear(gmx_ws, O, 1, m, d, 1, nullptr, nullptr, 0, gx, d, rows, O, d, 0, 1, stream)) return rc;
    if (!gm) return 0;
    STT_HIP(hipMemsetAsync(gm, 0, sizeof(float) * (size_t)O * d, s));
    if (int rc = sttode_twgrad(gmx_ws, O, x, d, 1, gm, d, nullptr, rows, O, d, mx_ws, (long)rows * O, stream)) return rc;
    return sttode_twgrad_flush();   // (inside a sttode_twgrad_defer bracket the split sums would otherwise be added later)
}

extern "C" int sttode_pmath_matvec_bwd(const float* m, const float* x, const float* g, float* mx_ws, float* gmx_ws, float* gxn_ws, float* gx,
                                       float* gm, int rows, int d, int O, float c, void* stream) {
    return pmath_matvec_bwd("sttode_pmath_matvec_bwd", m, x, g, mx_ws, gmx_ws, gxn_ws, gx, gm, rows, d, O, curv_float(c), stream);
}

extern "C" int sttode_pmath_matvec_bwd_c(const float* m, const float* x, const float* g, float* mx_ws, float* gmx_ws, float* gxn_ws, float* gx,
                                         float* gm, int rows, int d, int O, const float* c_dev, double* gc_ws, float* gc, void* stream) {
    return pmath_matvec_bwd("sttode_pmath_matvec_bwd_c", m, x, g, mx_ws, gmx_ws, gxn_ws, gx, gm, rows, d, O, curv_dev(c_dev, gc_ws, gc), stream);
}

// dist_matrix backward.  Device form: gc_ws holds P doubles (the side-0 pass, one wave per x row, sums its partners' shares; the side-1
// pass carries no share of dL/dc).  gx and gy may each be NULL; the side-1 pass runs only for gy.
static int pmath_dist_matrix_bwd(const char* who, const float* x, const float* y, const float* g, float* gx, float* gy, int P, int R, int d,
                                 Curv cv, void* stream) {
    PM_REQUIRE_CURV();
    PM_REQUIRE(x && y && g && (cv.dev || (gx && gy)), "null pointer");
    PM_REQUIRE(!cv.dev || (cv.gc_ws && cv.gc), "gc_ws [P] doubles and gc [1] are required");
    PM_REQUIRE(P > 0 && R > 0 && d > 0, "P, R, d must be positive");
    PM_REQUIRE(cv.dev || cv.c > 0.f, "curvature c must be positive");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((!cv.dev ? pmath_dist_matrix_bwd_kernel<false, false> : pmath_dist_matrix_bwd_kernel<true, true>), dim3((P + 3) / 4),
                       dim3(256), 0, s, 0, x, y, g, gx, P, R, d, cv.c, cv.c_dev, cv.gc_ws);
    if (gy)
        hipLaunchKernelGGL((!cv.dev ? pmath_dist_matrix_bwd_kernel<false, false> : pmath_dist_matrix_bwd_kernel<false, true>), dim3((R + 3) / 4),
                           dim3(256), 0, s, 1, x, y, g, gy, P, R, d, cv.c, cv.c_dev, (double*)nullptr);
    if (cv.dev) hipLaunchKernelGGL(pmath_gc_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)cv.gc_ws, cv.gc, (long)P);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_pmath_dist_matrix_bwd(const float* x, const float* y, const float* g, float* gx, float* gy, int P, int R, int d, float c,
                                            void* stream) {
    return pmath_dist_matrix_bwd("sttode_pmath_dist_matrix_bwd", x, y, g, gx, gy, P, R, d, curv_float(c), stream);
}

extern "C" int sttode_pmath_dist_matrix_bwd_c(const float* x, const float* y, const float* g, float* gx, float* gy, int P, int R, int d,
                                              const float* c_dev, double* gc_ws, float* gc, void* stream) {
    return pmath_dist_matrix_bwd("sttode_pmath_dist_matrix_bwd_c", x, y, g, gx, gy, P, R, d, curv_dev(c_dev, gc_ws, gc), stream);
}

// _hyperbolic_softmax backward: X [B,d], A [C,d], P [C,d], g [B,C] -> gX [B,d], gA [C,d], gP [C,d]; coef_ws [6,B,C] doubles.  Three launches
// (coefficients once per pair, then one wave per X row and one wave per class row); bitwise repeatable.  Device form: coef_ws holds
// SEVEN planes [7,B,C] (the seventh: g d logit / dc), gc_ws B doubles (the X-row pass sums the seventh plane over the classes).  gX may
// be NULL; gA and gP may be NULL together (then the class-row pass, which carries no share of dL/dc, is not run).
static int pmath_hsoftmax_bwd(const char* who, const float* X, const float* A, const float* P, const float* g, double* coef_ws, float* gX,
                              float* gA, float* gP, int B, int C, int d, Curv cv, void* stream) {
    PM_REQUIRE_CURV();
    PM_REQUIRE(X && A && P && g && coef_ws && (cv.dev || (gX && gA && gP)), "null pointer");
    PM_REQUIRE(!gA == !gP, "gA and gP are given together or not at all");
    PM_REQUIRE(!cv.dev || (cv.gc_ws && cv.gc), "gc_ws [B] doubles and gc [1] are required");
    PM_REQUIRE(B > 0 && C > 0 && d > 0, "B, C, d must be positive");
    PM_REQUIRE((long)B * C <= 0x7fffffffL, "more than 2^31 - 1 pairs");
    PM_REQUIRE(cv.dev || cv.c > 0.f, "curvature c must be positive");
    hipStream_t s = (hipStream_t)stream;
    const long BC = (long)B * C;
    auto coef = pmath_hsoftmax_coef_kernel<false>;
    auto xrows = pmath_hsoftmax_rowsum_kernel<false>;
    if (cv.dev) coef = pmath_hsoftmax_coef_kernel<true>, xrows = pmath_hsoftmax_rowsum_kernel<true>;
    hipLaunchKernelGGL(coef, dim3((unsigned)((BC + 3) / 4)), dim3(256), 0, s, X, A, P, g, coef_ws, B, C, d, cv.c, cv.c_dev);
    hipLaunchKernelGGL(xrows, dim3((B + 3) / 4), dim3(256), 0, s, 0, X, A, P, (const double*)coef_ws, gX, gA, gP, B, C, d, cv.gc_ws);
    if (gA)
        hipLaunchKernelGGL(pmath_hsoftmax_rowsum_kernel<false>, dim3((C + 3) / 4), dim3(256), 0, s, 1, X, A, P, (const double*)coef_ws, gX, gA, gP,
                           B, C, d, (double*)nullptr);
    if (cv.dev) hipLaunchKernelGGL(pmath_gc_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)cv.gc_ws, cv.gc, (long)B);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_pmath_hsoftmax_bwd(const float* X, const float* A, const float* P, const float* g, double* coef_ws, float* gX, float* gA,
                                         float* gP, int B, int C, int d, float c, void* stream) {
    return pmath_hsoftmax_bwd("sttode_pmath_hsoftmax_bwd", X, A, P, g, coef_ws, gX, gA, gP, B, C, d, curv_float(c), stream);
}

extern "C" int sttode_pmath_hsoftmax_bwd_c(const float* X, const float* A, const float* P, const float* g, double* coef_ws, float* gX, float* gA,
                                           float* gP, int B, int C, int d, const float* c_dev, double* gc_ws, float* gc, void* stream) {
    return pmath_hsoftmax_bwd("sttode_pmath_hsoftmax_bwd_c", X, A, P, g, coef_ws, gX, gA, gP, B, C, d, curv_dev(c_dev, gc_ws, gc), stream);
}

// Feature clipping x min(1, r / (|x| + 1e-5)) over rows (ToPoincare(clip_r=r)) and its backward pass.
extern "C" int sttode_pmath_clip(const float* x, float* out, int rows, int d, float r, void* stream) {
    STT_REQUIRE(x && out && rows > 0 && d > 0, "sttode_pmath_clip: null pointer or empty shape");
    STT_REQUIRE(r > 0.f, "sttode_pmath_clip: the clipping radius r must be positive");
    hipLaunchKernelGGL(pmath_clip_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, out, rows, d, r);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_pmath_clip_bwd(const float* x, const float* g, float* gx, int rows, int d, float r, void* stream) {
    STT_REQUIRE(x && g && gx && rows > 0 && d > 0, "sttode_pmath_clip_bwd: null pointer or empty shape");
    STT_REQUIRE(r > 0.f, "sttode_pmath_clip_bwd: the clipping radius r must be positive");
    hipLaunchKernelGGL(pmath_clip_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, g, gx, rows, d, r);
    STT_HIP(hipGetLastError());
    return 0;
}
