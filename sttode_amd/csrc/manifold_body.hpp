// Per-row device functions of the manifolds the Riemannian optimisers step on (csrc/manifold.hip), one set per manifold code:
//   MF_EUCLIDEAN   core/manifolds/euclidean.py: identities and adds
//   MF_OBLIQUE     core/manifolds/oblique.py: rows of unit norm
//   MF_POINCARE    the Poincare ball of curvature -c that pmath.hip works on (hyptorch/pmath.py)
// Every operation of the interface maps rows to a LINEAR COMBINATION OF ITS OPERAND ROWS whose coefficients depend only on the row's dot
// products: egrad2rgrad(x, g) = cg g + cx x, expmap(u, x) = cx x + cu u, retr = k expmap, ptransp(x, y, w) = cw w + cy y + cx x,
// inner_x(u, v) = s <u, v>.  The functions below return those coefficients from the wave-reduced dot products, in float64: 1 - c |x|^2 and
// the gyration's denominator cancel near the ball boundary, and the Oblique tangent projection cancels when g is nearly parallel to x.
// Both the row-op kernel and the optimiser-step kernel are built from these functions and nothing else, so the op tests cover the step.
// A dot product with a result of these functions (|y|^2, <y, w>, ...) is a quadratic form in the dot products of the operands: the step
// kernel reads every row once, forms six sums, and writes the new row.
// The coefficient functions are templates over their scalar type T: T = double is the arithmetic of the forward and
// optimiser kernels; T = DN<N> (dual.hpp) carries the partial derivatives with respect to the row's dot products through the same
// formulas, which is what the backward kernel of the row ops is built from.  c is a constant in both.  Branches differentiate as taken;
// a clamp passes the gradient where its argument is inside (bounds included), a norm has derivative 0 at a zero row.
#pragma once
#include <hip/hip_runtime.h>
#include "dual.hpp"

enum MfManifold { MF_EUCLIDEAN = 0, MF_OBLIQUE = 1, MF_POINCARE = 2, MF_COUNT };

#define MF_OBL_EPS 1e-4      // EPS[torch.float32] of core/manifolds/oblique.py:7: below it expmap is proj(p + u)
#define MF_MIN_NORM 1e-5     // hyptorch/pmath.py's clamp_min(1e-5) of norms and the + 1e-5 of the Moebius denominator
#define MF_BALL_EPS 1e-3     // project (pmath.py:98-103): maxnorm = (1 - 1e-3) / sqrt(c)

template <class T> struct MfLin2T { T a, b; };       // a * (first operand) + b * (second operand)
template <class T> struct MfLin3T { T w, y, x; };    // ptransp(x, y, w) = w * w_row + y * y_row + x * x_row
using MfLin2 = MfLin2T<double>;
using MfLin3 = MfLin3T<double>;

// the primitives of the formulas below, for both scalar types
template <class T> struct MfK;                                      // a constant as a T
template <> struct MfK<double> { static __device__ __forceinline__ double of(double v) { return v; } };
template <int N> struct MfK<DN<N>> { static __device__ __forceinline__ DN<N> of(double v) { return cst<N>(v); } };
__device__ __forceinline__ double mf_val(double a) { return a; }
template <int N> __device__ __forceinline__ double mf_val(const DN<N>& a) { return a.v; }
__device__ __forceinline__ double mf_sqrt(double a) { return sqrt(a); }
template <int N> __device__ __forceinline__ DN<N> mf_sqrt(const DN<N>& a) { return norm_of(a); }
__device__ __forceinline__ double mf_cos(double a) { return cos(a); }
template <int N> __device__ __forceinline__ DN<N> mf_cos(const DN<N>& a) { return chain(cos(a.v), -sin(a.v), a); }
__device__ __forceinline__ double mf_sin(double a) { return sin(a); }
template <int N> __device__ __forceinline__ DN<N> mf_sin(const DN<N>& a) { return chain(sin(a.v), cos(a.v), a); }
__device__ __forceinline__ double mf_clamp_min(double a, double lo) { return fmax(a, lo); }
template <int N> __device__ __forceinline__ DN<N> mf_clamp_min(const DN<N>& a, double lo) { return clamp_min_(a, lo); }
__device__ __forceinline__ double mf_tanh15(double a) { return tanh(fmin(fmax(a, -15.0), 15.0)); }
template <int N> __device__ __forceinline__ DN<N> mf_tanh15(const DN<N>& a) { return tanh_clamped_(a); }

__device__ __forceinline__ double mf_wsum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float mf_wsumf(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// egrad2rgrad(x, g) = a g + b x from x2 = |x|^2, xg = <x, g>.  Oblique: proj_tan (oblique.py:18-20, :64-65); ball: g / lambda_x^2, the
// scale of RiemannianGradient (pmath.py:39-45).
template <class T> __device__ __forceinline__ MfLin2T<T> mf_egrad2rgrad(int man, double c, T x2, T xg) {
    if (man == MF_OBLIQUE) return MfLin2T<T>{MfK<T>::of(1.0), -xg};
    if (man == MF_POINCARE) { const T t = 1.0 - c * x2; return MfLin2T<T>{t * t * 0.25, MfK<T>::of(0.0)}; }
    return MfLin2T<T>{MfK<T>::of(1.0), MfK<T>::of(0.0)};
}

// inner_x(u, v) = s <u, v>: lambda_x^2 on the ball, 1 otherwise
template <class T> __device__ __forceinline__ T mf_inner_scale(int man, double c, T x2) {
    if (man != MF_POINCARE) return MfK<T>::of(1.0);
    const T lam = 2.0 / (1.0 - c * x2);
    return lam * lam;
}

// expmap(u, x) = a x + b u from x2, u2 = |u|^2, xu = <x, u>, before any projection.
//   Oblique (oblique.py:22-27): x cos|u| + u sin|u| / |u| for |u| > 1e-4, else (x + u) / |x + u| (a zero u gives x / |x|, not NaN);
//   ball (pmath.py:268-277): x (+) tanh(sqrt_c lambda_x |u| / 2) u / (sqrt_c |u|), the reference's clamps and its + 1e-5 kept.
template <class T> __device__ __forceinline__ MfLin2T<T> mf_expmap(int man, double c, T x2, T u2, T xu) {
    if (man == MF_OBLIQUE) {
        const T un = mf_sqrt(u2);
        if (mf_val(un) > MF_OBL_EPS) return MfLin2T<T>{mf_cos(un), mf_sin(un) / un};
        const T n = mf_sqrt(x2 + 2.0 * xu + u2);
        return MfLin2T<T>{1.0 / n, 1.0 / n};
    }
    if (man == MF_POINCARE) {
        const double sc = sqrt(c);
        const T un = mf_clamp_min(mf_sqrt(u2), MF_MIN_NORM), lam = 2.0 / (1.0 - c * x2);
        const T s = mf_tanh15(sc * 0.5 * lam * un) / (sc * un);   // second_term = s u
        const T b2 = s * s * u2, ab = s * xu;
        const T den = 1.0 + 2.0 * c * ab + c * c * x2 * b2 + MF_MIN_NORM;
        return MfLin2T<T>{(1.0 + 2.0 * c * ab + c * b2) / den, (1.0 - c * x2) * s / den};
    }
    return MfLin2T<T>{MfK<T>::of(1.0), MfK<T>::of(1.0)};
}

// retr(x, u) = k expmap(u, x): the factor k from y2 = |expmap|^2.  Oblique: the renormalisation 1 / |y| (the identity in exact arithmetic:
// it keeps fp32 rows on the sphere over thousands of steps); ball: project, whose branch is taken by the forward kernel's own fp32 test
// (pmath.hip OP_PROJECT) on y2f, the fp32 sum of squares of the fp32-rounded row in that kernel's order, so that pmath.project of the
// stored row takes the same branch.
template <class T> __device__ __forceinline__ T mf_retr_scale(int man, double c, T y2, float y2f) {
    if (man == MF_OBLIQUE) return 1.0 / mf_sqrt(y2);
    if (man == MF_POINCARE) {
        const float normf = fmaxf(sqrtf(y2f), 1e-5f), maxnormf = (1.0f - 1e-3f) / sqrtf((float)c);
        return normf > maxnormf ? ((1.0 - MF_BALL_EPS) / sqrt(c)) / mf_clamp_min(mf_sqrt(y2), MF_MIN_NORM) : MfK<T>::of(1.0);
    }
    return MfK<T>::of(1.0);
}

// ptransp(x, y, w) from x2, y2, xy = <x, y>, xw = <x, w>, yw = <y, w>.  Oblique (oblique.py:60-62): proj_tan(w, y).  Ball:
// gyr[y, -x] w lambda_x / lambda_y with the gyration in closed form, k = -c: gyr[a, b] w = w + 2 (A a + B b) / D,
//   A = -k^2 <a,w> |b|^2 - k <b,w> + 2 k^2 <a,b> <b,w>,   B = -k^2 <b,w> |a|^2 + k <a,w>,   D = 1 - 2 k <a,b> + k^2 |a|^2 |b|^2.
template <class T> __device__ __forceinline__ MfLin3T<T> mf_ptransp(int man, double c, T x2, T y2, T xy, T xw, T yw) {
    if (man == MF_OBLIQUE) return MfLin3T<T>{MfK<T>::of(1.0), -yw, MfK<T>::of(0.0)};
    if (man == MF_POINCARE) {
        const double k = -c, k2 = c * c;
        const T u2 = y2, v2 = x2, uv = -xy, uw = yw, vw = -xw;             // a = y, b = -x
        const T A = -k2 * uw * v2 - k * vw + 2.0 * k2 * uv * vw;
        const T B = -k2 * vw * u2 + k * uw;
        const T D = 1.0 - 2.0 * k * uv + k2 * u2 * v2;
        const T s = (1.0 - c * y2) / (1.0 - c * x2);                       // lambda_x / lambda_y
        return MfLin3T<T>{s, s * 2.0 * A / D, -s * 2.0 * B / D};
    }
    return MfLin3T<T>{MfK<T>::of(1.0), MfK<T>::of(0.0), MfK<T>::of(0.0)};
}
