// Float64 forward-mode arithmetic for the scalar stages of the backward kernels (csrc/pmath_grad.hip, csrc/manifold.hip): struct DN<N> is a
// value and N partials.  The primitives carry the derivative that the reference's autograd gives, not the textbook one (the list stands at
// the head of pmath_grad.hip).
#pragma once
#include <hip/hip_runtime.h>

constexpr double EPS5 = (double)1e-5f;   // the reference's 1e-5, as the forward kernels round it

// value + partials with respect to N scalars (D3: the three row scalars; D6: the six pair scalars of _hyperbolic_softmax)
template <int N> struct DN { double v, d[N]; };
using D3 = DN<3>;
using D6 = DN<6>;
// the value v with partials d[k] = f(k)
template <int N, class F> __device__ __forceinline__ DN<N> dn(double v, F f) {
    DN<N> r; r.v = v;
#pragma unroll
    for (int k = 0; k < N; ++k) r.d[k] = f(k);
    return r;
}
template <int N> __device__ __forceinline__ DN<N> cst(double v) { return dn<N>(v, [](int) { return 0.; }); }
template <int N> __device__ __forceinline__ DN<N> var(double v, int i) { return dn<N>(v, [i](int k) { return k == i ? 1. : 0.; }); }
template <int N> __device__ __forceinline__ DN<N> operator+(const DN<N>& a, const DN<N>& b) { return dn<N>(a.v + b.v, [&](int k) { return a.d[k] + b.d[k]; }); }
template <int N> __device__ __forceinline__ DN<N> operator-(const DN<N>& a, const DN<N>& b) { return dn<N>(a.v - b.v, [&](int k) { return a.d[k] - b.d[k]; }); }
template <int N> __device__ __forceinline__ DN<N> operator-(const DN<N>& a) { return dn<N>(-a.v, [&](int k) { return -a.d[k]; }); }
template <int N> __device__ __forceinline__ DN<N> operator*(const DN<N>& a, const DN<N>& b) {
    return dn<N>(a.v * b.v, [&](int k) { return a.d[k] * b.v + a.v * b.d[k]; });
}
template <int N> __device__ __forceinline__ DN<N> operator/(const DN<N>& a, const DN<N>& b) {
    const double q = a.v / b.v, ib = 1.0 / b.v;
    return dn<N>(q, [&](int k) { return (a.d[k] - q * b.d[k]) * ib; });
}
template <int N> __device__ __forceinline__ DN<N> operator+(double a, const DN<N>& b) { return dn<N>(a + b.v, [&](int k) { return b.d[k]; }); }
template <int N> __device__ __forceinline__ DN<N> operator-(double a, const DN<N>& b) { return dn<N>(a - b.v, [&](int k) { return -b.d[k]; }); }
template <int N> __device__ __forceinline__ DN<N> operator*(double a, const DN<N>& b) { return dn<N>(a * b.v, [&](int k) { return a * b.d[k]; }); }
template <int N> __device__ __forceinline__ DN<N> operator/(double a, const DN<N>& b) { return cst<N>(a) / b; }
template <int N> __device__ __forceinline__ DN<N> operator+(const DN<N>& a, double b) { return b + a; }
template <int N> __device__ __forceinline__ DN<N> operator-(const DN<N>& a, double b) { return dn<N>(a.v - b, [&](int k) { return a.d[k]; }); }
template <int N> __device__ __forceinline__ DN<N> operator*(const DN<N>& a, double b) { return b * a; }
template <int N> __device__ __forceinline__ DN<N> operator/(const DN<N>& a, double b) { return (1.0 / b) * a; }
template <int N> __device__ __forceinline__ DN<N> chain(double v, double dv, const DN<N>& a) { return dn<N>(v, [&](int k) { return dv * a.d[k]; }); }
// x.norm(): sqrt of a sum of squares, derivative 0 at a zero row
template <int N> __device__ __forceinline__ DN<N> norm_of(const DN<N>& sq) { const double n = sqrt(sq.v); return chain(n, n > 0. ? 0.5 / n : 0., sq); }
template <int N> __device__ __forceinline__ DN<N> sqrt_(const DN<N>& a) { const double n = sqrt(a.v); return chain(n, 0.5 / n, a); }
template <int N> __device__ __forceinline__ DN<N> clamp_min_(const DN<N>& a, double lo) { return a.v >= lo ? a : cst<N>(lo); }
template <int N> __device__ __forceinline__ DN<N> tanh_clamped_(const DN<N>& a) {   // pmath.py:11-12
    const bool in = a.v >= -15.0 && a.v <= 15.0;
    const double t = tanh(fmin(fmax(a.v, -15.0), 15.0));
    return chain(t, in ? 1.0 - t * t : 0., a);
}
template <int N> __device__ __forceinline__ DN<N> artanh_d(const DN<N>& a) {        // pmath.py:16-27
    const double xc = fmin(fmax(a.v, -1.0 + EPS5), 1.0 - EPS5);
    return chain(0.5 * (log1p(xc) - log1p(-xc)), 1.0 / (1.0 - xc * xc), a);
}
// arsinh (pmath.py:51-60): log of the clamped x + sqrt(1 + x^2); the derivative Arsinh.backward gives, 1 / sqrt(1 + x^2), whatever the clamp
template <int N> __device__ __forceinline__ DN<N> arsinh_d(const DN<N>& a) {
    const double h = sqrt(1.0 + a.v * a.v);
    return chain(log(fmax(a.v + h, EPS5)), 1.0 / h, a);
}
