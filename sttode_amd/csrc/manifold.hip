// Riemannian optimisation on the device: the row operations of the manifold interface of core/manifolds (base.py: egrad2rgrad,
// proj_tan, expmap, ptransp, retr, retr_transp, inner) for the Euclidean, Oblique and Poincare-ball manifolds, and Riemannian Adam / SGD over
// ALL manifold parameters of a param group in ONE launch.  The reference declares the interface and ships no optimiser that uses it.
//
//   manifold_row_kernel      one op on rows of [rows, d] operands (sttode_manifold_rowop)
//   riemannian_step_kernel   g += wd x; r = egrad2rgrad(x, g); moments; y = retr(x, -lr dir); m = ptransp(x, y, m); x = y, per row, for every
//                            parameter of a device table (sttode_riemannian_step)
//   riemannian_tick_kernel   one thread: the device step count + 1 (only in front of a step that reads its count from the device: a
//                            captured step, whose host arguments are frozen)
// ONE WAVE PER ROW (the step kernel: two or four rows per wave at d <= 32, d <= 16), four waves per 256-thread block, as pmath.hip and
// pmath_grad.hip: d is in the tens to hundreds, a row is one or a few
// coalesced 256-byte requests per operand, and its dot products are a 6-step xor-shuffle with no LDS and no barrier.  Every result row is a
// linear combination of the operand rows (manifold_body.hpp), so a kernel is: pass 1, the dot products of the operands in float64; the
// scalar stage, redundantly on all lanes; pass 2, the combination, written with plain coalesced stores.  The ball's retraction has one
// more pass over the row (from cache) for project's fp32 clip test.  No atomics, no LDS, no workspace, nothing allocated; every sum has a
// fixed order, so results repeat bit for bit.
#include "api_util.hpp"
#include "manifold_body.hpp"
#include "../../include/sttode_hip.h"
#include <cmath>

namespace {

enum { MOP_PROJ_TAN = 0, MOP_EXPMAP, MOP_PTRANSP, MOP_INNER, MOP_RETR, MOP_RETR_TRANSP, MOP_COUNT };   // enum SttodeManifoldOp
enum { RULE_ADAM = 0, RULE_SGD = 1, RULE_COUNT };                                                     // enum SttodeRiemannianRule

// ---- row ops --------------------------------------------------------------------------------------------------------------------------
// operands (a, b, w):  proj_tan / egrad2rgrad (p, u, -)   expmap, retr (p, u, -)   ptransp (x, y, u)   inner (p, u, v or NULL: v = u)
//                      retr_transp (x, u, v) -> out = y, out2 = ptransp(x, y, v)
__global__ __launch_bounds__(256) void manifold_row_kernel(int op, int man, const float* __restrict__ a, const float* __restrict__ b,
                                                           const float* __restrict__ w, float* __restrict__ out, float* __restrict__ out2,
                                                           int rows, int d, double c) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* ar = a + (size_t)r * d;
    const float* br = b + (size_t)r * d;
    const float* wr = w ? w + (size_t)r * d : nullptr;
    double a2 = 0., b2 = 0., ab = 0., aw = 0., bw = 0.;
    for (int i = lane; i < d; i += 64) {
        const double x = ar[i], y = br[i];
        a2 += x * x; b2 += y * y; ab += x * y;
        if (wr) { const double z = wr[i]; aw += x * z; bw += y * z; }
    }
    a2 = mf_wsum(a2); b2 = mf_wsum(b2); ab = mf_wsum(ab); aw = mf_wsum(aw); bw = mf_wsum(bw);
    float* o = out + (size_t)r * d;
    switch (op) {
        case MOP_PROJ_TAN: {
            const MfLin2 e = mf_egrad2rgrad(man, c, a2, ab);
            for (int i = lane; i < d; i += 64) o[i] = (float)(e.a * (double)br[i] + e.b * (double)ar[i]);
        } break;
        case MOP_EXPMAP: {
            const MfLin2 e = mf_expmap(man, c, a2, b2, ab);
            for (int i = lane; i < d; i += 64) o[i] = (float)(e.a * (double)ar[i] + e.b * (double)br[i]);
        } break;
        case MOP_PTRANSP: {
            const MfLin3 p = mf_ptransp(man, c, a2, b2, ab, aw, bw);
            for (int i = lane; i < d; i += 64) o[i] = (float)(p.w * (double)wr[i] + p.y * (double)br[i] + p.x * (double)ar[i]);
        } break;
        case MOP_INNER:
            if (lane == 0) out[r] = (float)(mf_inner_scale(man, c, a2) * (wr ? bw : b2));
            break;
        default: {   // MOP_RETR, MOP_RETR_TRANSP
            const MfLin2 e = mf_expmap(man, c, a2, b2, ab);
            float y2f = 0.f;
            if (man == MF_POINCARE) {
                for (int i = lane; i < d; i += 64) { const float y = (float)(e.a * (double)ar[i] + e.b * (double)br[i]); y2f += y * y; }
                y2f = mf_wsumf(y2f);
            }
            const double k = mf_retr_scale(man, c, e.a * e.a * a2 + 2.0 * e.a * e.b * ab + e.b * e.b * b2, y2f);
            const double ya = k * e.a, yb = k * e.b;                        // y = ya x + yb u
            for (int i = lane; i < d; i += 64) o[i] = (float)(ya * (double)ar[i] + yb * (double)br[i]);
            if (op == MOP_RETR_TRANSP) {
                const double y2 = ya * ya * a2 + 2.0 * ya * yb * ab + yb * yb * b2, xy = ya * a2 + yb * ab, yw = ya * aw + yb * bw;
                const MfLin3 p = mf_ptransp(man, c, a2, y2, xy, aw, yw);
                float* o2 = out2 + (size_t)r * d;
                for (int i = lane; i < d; i += 64) {
                    const double x = ar[i], u = br[i];
                    o2[i] = (float)(p.w * (double)wr[i] + p.y * (ya * x + yb * u) + p.x * x);
                }
            }
        } break;
    }
}

// ---- row ops, backward ---------------------------------------------------------------------------------------------------
// Every forward row is out = ca a + cb b + cw w (retr_transp: a second row out2 of the same form) with coefficients that are functions of
// the five dot products p = (|a|^2, |b|^2, <a,b>, <a,w>, <b,w>).  With T_j = sum_k dc_k/dp_j <g, operand_k> (and the same over out2's
// coefficients and g2) the vector-Jacobian product is
//     ga = ca g + 2 T_0 a + T_2 b + T_3 w,   gb = cb g + 2 T_1 b + T_2 a + T_4 w,   gw = cw g + T_3 a + T_4 b
// (inner: the scalar f(p) in place of the coefficients, T_j = g df/dp_j, no c g terms).  The coefficients and their partials come from
// the forward's own mf_* functions evaluated on DN<5>: the gyration, the clamps and the branches are differentiated as the forward took
// them, with no second formula to keep in step.  The ball's retraction takes project's branch by the forward kernel's fp32 test.
// ONE WAVE PER ROW as the forward: pass 1, the five dot products and the operands' dot products with g and g2 in float64; the scalar
// stage; pass 2, the three gradient rows with plain coalesced stores.  ONE launch, no atomics, no workspace; every sum in a fixed order.
using D5 = DN<5>;
struct MfCoef { D5 a, b, w; };   // a row as ca a + cb b + cw w

__global__ __launch_bounds__(256) void manifold_row_bwd_kernel(int op, int man, const float* __restrict__ a, const float* __restrict__ b,
                                                               const float* __restrict__ w, const float* __restrict__ g,
                                                               const float* __restrict__ g2, float* __restrict__ ga, float* __restrict__ gb,
                                                               float* __restrict__ gw, int rows, int d, double c) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const bool scalar = op == MOP_INNER;
    const float* ar = a + (size_t)r * d;
    const float* br = b + (size_t)r * d;
    const float* wr = w ? w + (size_t)r * d : nullptr;
    const float* gr = g && !scalar ? g + (size_t)r * d : nullptr;
    const float* hr = g2 ? g2 + (size_t)r * d : nullptr;
    double a2 = 0., b2 = 0., ab = 0., aw = 0., bw = 0., ga_ = 0., gb_ = 0., gw_ = 0., ha_ = 0., hb_ = 0., hw_ = 0.;
    for (int i = lane; i < d; i += 64) {
        const double x = ar[i], y = br[i], z = wr ? (double)wr[i] : 0., gi = gr ? (double)gr[i] : 0., hi = hr ? (double)hr[i] : 0.;
        a2 += x * x; b2 += y * y; ab += x * y; aw += x * z; bw += y * z;
        ga_ += gi * x; gb_ += gi * y; gw_ += gi * z; ha_ += hi * x; hb_ += hi * y; hw_ += hi * z;
    }
    a2 = mf_wsum(a2); b2 = mf_wsum(b2); ab = mf_wsum(ab); aw = mf_wsum(aw); bw = mf_wsum(bw);
    ga_ = mf_wsum(ga_); gb_ = mf_wsum(gb_); gw_ = mf_wsum(gw_); ha_ = mf_wsum(ha_); hb_ = mf_wsum(hb_); hw_ = mf_wsum(hw_);
    const D5 A2 = var<5>(a2, 0), B2 = var<5>(b2, 1), AB = var<5>(ab, 2), AW = var<5>(aw, 3), BW = var<5>(bw, 4), Z = cst<5>(0.);
    MfCoef c1 = {Z, Z, Z}, c2 = {Z, Z, Z};
    double T[5];
    switch (op) {
        case MOP_PROJ_TAN: { const MfLin2T<D5> e = mf_egrad2rgrad(man, c, A2, AB); c1.a = e.b; c1.b = e.a; } break;
        case MOP_EXPMAP: { const MfLin2T<D5> e = mf_expmap(man, c, A2, B2, AB); c1.a = e.a; c1.b = e.b; } break;
        case MOP_PTRANSP: { const MfLin3T<D5> p = mf_ptransp(man, c, A2, B2, AB, AW, BW); c1.a = p.x; c1.b = p.y; c1.w = p.w; } break;
        case MOP_INNER: c1.a = mf_inner_scale(man, c, A2) * (wr ? BW : B2); break;   // the scalar f(p)
        default: {   // MOP_RETR, MOP_RETR_TRANSP
            const MfLin2T<D5> e = mf_expmap(man, c, A2, B2, AB);
            float y2f = 0.f;
            if (man == MF_POINCARE) {   // the forward kernel's own test, on the row it rounded
                for (int i = lane; i < d; i += 64) { const float y = (float)(e.a.v * (double)ar[i] + e.b.v * (double)br[i]); y2f += y * y; }
                y2f = mf_wsumf(y2f);
            }
            const D5 k = mf_retr_scale(man, c, e.a * e.a * A2 + 2.0 * e.a * e.b * AB + e.b * e.b * B2, y2f);
            const D5 ya = k * e.a, yb = k * e.b;
            c1.a = ya; c1.b = yb;
            if (op == MOP_RETR_TRANSP) {
                const D5 y2 = ya * ya * A2 + 2.0 * ya * yb * AB + yb * yb * B2, xy = ya * A2 + yb * AB, yw = ya * AW + yb * BW;
                const MfLin3T<D5> p = mf_ptransp(man, c, A2, y2, xy, AW, yw);
                c2.a = p.y * ya + p.x; c2.b = p.y * yb; c2.w = p.w;
            }
        } break;
    }
    double ka = 0., kb = 0., kw = 0., ha = 0., hb = 0., hw = 0.;   // the factors of g and g2 in ga, gb, gw
    if (scalar) {
        const double gs = g[r];
#pragma unroll
        for (int j = 0; j < 5; ++j) T[j] = gs * c1.a.d[j];
    } else {
#pragma unroll
        for (int j = 0; j < 5; ++j)
            T[j] = c1.a.d[j] * ga_ + c1.b.d[j] * gb_ + c1.w.d[j] * gw_ + c2.a.d[j] * ha_ + c2.b.d[j] * hb_ + c2.w.d[j] * hw_;
        ka = c1.a.v; kb = c1.b.v; kw = c1.w.v; ha = c2.a.v; hb = c2.b.v; hw = c2.w.v;
    }
    float* gar = ga ? ga + (size_t)r * d : nullptr;
    float* gbr = gb ? gb + (size_t)r * d : nullptr;
    float* gwr = gw && wr ? gw + (size_t)r * d : nullptr;
    for (int i = lane; i < d; i += 64) {
        const double x = ar[i], y = br[i], z = wr ? (double)wr[i] : 0., gi = gr ? (double)gr[i] : 0., hi = hr ? (double)hr[i] : 0.;
        if (gar) gar[i] = (float)(ka * gi + ha * hi + 2.0 * T[0] * x + T[2] * y + T[3] * z);
        if (gbr) gbr[i] = (float)(kb * gi + hb * hi + 2.0 * T[1] * y + T[2] * x + T[4] * z);
        if (gwr) gwr[i] = (float)(kw * gi + hw * hi + T[3] * x + T[4] * y);
    }
}

// ---- the optimiser step -------------------------------------------------------------------------------------------------------------------
// One row of the device table per parameter (10 x 8 bytes): the parameter, its two state buffers (Adam: exp_avg [rows, d], exp_avg_sq
// [rows]; SGD: momentum_buffer or NULL, unused), its gradient, the row length d, the row count, the first wave slot (ascending from 0), the
// manifold code, c, and the element count (rows d for a manifold parameter; a plain parameter is cut into rows of d elements whose last one
// may be short).
// A WAVE SLOT is what one wave steps: one row on 64 lanes for d > 32, two rows on 32 lanes each for d <= 32, four rows on 16 lanes each
// for d <= 16 (riem_group).  The per-row scalar stage is some hundreds of float64 instructions that every lane runs whatever it holds; at
// d = 16 a row fills a quarter of a wave, so four rows share one pass through that stage.  A parameter takes ceil(rows / rows per slot) slots.
struct RiemItem { float* p; float* m; float* v; const float* g; long d; long rows; long slot0; long manifold; double c; long numel; };
static_assert(sizeof(RiemItem) == 8 * STTODE_RIEMANNIAN_ITEM_WORDS, "table row layout");

__host__ __device__ __forceinline__ int riem_group(long d) { return d <= 16 ? 16 : d <= 32 ? 32 : 64; }   // lanes per row

// sum over the aligned group of G lanes (G = 16, 32 or 64) a lane belongs to
__device__ __forceinline__ double mf_gsum(double v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float mf_gsumf(float v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the parameter of wave slot S: largest t with slot0[t] <= S
__device__ __forceinline__ RiemItem riem_item_of(const RiemItem* __restrict__ items, int n, long S) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].slot0 <= S) lo = mid; else hi = mid - 1;
    }
    return items[lo];
}

// a row as a combination m_c m + g_c g + x_c x of the three rows the step reads, and the dot product of two such rows from the Gram matrix
struct V3 { double m, g, x; };
struct Gram { double mm, gg, xx, mg, mx, gx; };
__device__ __forceinline__ double dot3(const V3& a, const V3& b, const Gram& G) {
    return a.m * b.m * G.mm + a.g * b.g * G.gg + a.x * b.x * G.xx + (a.m * b.g + a.g * b.m) * G.mg + (a.m * b.x + a.x * b.m) * G.mx +
           (a.g * b.x + a.x * b.g) * G.gx;
}
__device__ __forceinline__ double at3(const V3& a, double m, double g, double x) { return a.m * m + a.g * g + a.x * x; }

template <int RULE>
__global__ __launch_bounds__(256) void riemannian_step_kernel(const RiemItem* __restrict__ items, int n, long total_slots, double lr, double beta1,
                                                              double beta2, double eps, double wd, double mom, double t_host, double* tstate) {
    const int lane = threadIdx.x & 63;
    const long S = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (S >= total_slots) return;
    const RiemItem it = riem_item_of(items, n, S);
    if (it.d <= 0) return;
    const int L = riem_group(it.d), li = lane & (L - 1);               // L lanes per row, this lane's place among them
    const long r = (S - it.slot0) * (64 / L) + lane / L;
    // a group of lanes past the parameter's last row holds no row: it loads and stores nothing (len 0) and runs the scalar stage on zeros
    const bool live = r < it.rows && r * it.d < it.numel;
    const long off = live ? r * it.d : 0;
    const int len = live ? (int)(it.numel - off < it.d ? it.numel - off : it.d) : 0;
    const int man = (int)it.manifold;
    const double c = it.c;
    float* xr = it.p + off;
    const float* gr = it.g + off;
    float* mr = it.m ? it.m + off : nullptr;
    Gram G = {0., 0., 0., 0., 0., 0.};
    if (RULE == RULE_ADAM || man != MF_EUCLIDEAN) {      // (plain SGD rows are elementwise: no dot products)
        for (int i = li; i < len; i += L) {
            const double x = xr[i], g = gr[i], m = mr ? (double)mr[i] : 0.;
            G.mm += m * m; G.gg += g * g; G.xx += x * x; G.mg += m * g; G.mx += m * x; G.gx += g * x;
        }
        G.mm = mf_gsum(G.mm, L); G.gg = mf_gsum(G.gg, L); G.xx = mf_gsum(G.xx, L); G.mg = mf_gsum(G.mg, L); G.mx = mf_gsum(G.mx, L);
        G.gx = mf_gsum(G.gx, L);
    }
    const V3 X = {0., 0., 1.};
    // g += wd x; r = egrad2rgrad(x, g)
    const MfLin2 e = mf_egrad2rgrad(man, c, G.xx, G.gx + wd * G.xx);
    const V3 rg = {0., e.a, e.a * wd + e.b};
    V3 mn;            // the new first moment / momentum buffer, before transport
    double step;      // u = step * mn
    double vnew = 0.;
    if (RULE == RULE_ADAM) {
        double t = t_host;
        if (tstate) {
            if (t_host > 0.) { if (S == 0 && lane == 0) tstate[0] = t_host; }   // (keeps the device count in step with the host's)
            else t = tstate[0];
        }
        const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
        mn = V3{beta1, (1.0 - beta1) * rg.g, (1.0 - beta1) * rg.x};
        vnew = beta2 * (live ? (double)it.v[r] : 0.) + (1.0 - beta2) * mf_inner_scale(man, c, G.xx) * dot3(rg, rg, G);
        step = -lr / (bc1 * (sqrt(vnew / bc2) + eps));
    } else {
        mn = mr ? V3{mom, rg.g, rg.x} : rg;
        step = -lr;
    }
    // y = retr(x, u), u = step mn
    const V3 U = {step * mn.m, step * mn.g, step * mn.x};
    const MfLin2 ex = mf_expmap(man, c, G.xx, dot3(U, U, G), dot3(X, U, G));
    const V3 Y0 = {ex.b * U.m, ex.b * U.g, ex.b * U.x + ex.a};
    float y2f = 0.f;
    if (man == MF_POINCARE) {
        for (int i = li; i < len; i += L) {
            const float y = (float)at3(Y0, mr ? (double)mr[i] : 0., (double)gr[i], (double)xr[i]);
            y2f += y * y;
        }
        y2f = mf_gsumf(y2f, L);
    }
    const double k = mf_retr_scale(man, c, dot3(Y0, Y0, G), y2f);
    const V3 Y = {k * Y0.m, k * Y0.g, k * Y0.x};
    // m = ptransp(x, y, m)
    const MfLin3 pt = mf_ptransp(man, c, G.xx, dot3(Y, Y, G), dot3(X, Y, G), dot3(X, mn, G), dot3(Y, mn, G));
    const V3 MT = {pt.w * mn.m + pt.y * Y.m, pt.w * mn.g + pt.y * Y.g, pt.w * mn.x + pt.y * Y.x + pt.x};
    for (int i = li; i < len; i += L) {
        const double x = xr[i], g = gr[i], m = mr ? (double)mr[i] : 0.;
        xr[i] = (float)at3(Y, m, g, x);
        if (mr) mr[i] = (float)at3(MT, m, g, x);
    }
    if (RULE == RULE_ADAM && live && li == 0) it.v[r] = (float)vnew;
}

__global__ void riemannian_tick_kernel(double* tstate) { tstate[0] += 1.0; }

bool finite_(double v) { return std::isfinite(v); }

}  // namespace

extern "C" int sttode_manifold_rowop(int op, int manifold, const float* a, const float* b, const float* w, float* out, float* out2, int rows,
                                     int d, float c, void* stream) {
    STT_REQUIRE(op >= 0 && op < MOP_COUNT, "sttode_manifold_rowop: unknown op");
    STT_REQUIRE(manifold >= 0 && manifold < MF_COUNT, "sttode_manifold_rowop: unknown manifold");
    STT_REQUIRE(a && b && out, "sttode_manifold_rowop: null pointer");
    STT_REQUIRE(rows > 0 && d > 0, "sttode_manifold_rowop: empty shape");
    STT_REQUIRE(w || (op != MOP_PTRANSP && op != MOP_RETR_TRANSP), "sttode_manifold_rowop: this op needs the third operand");
    STT_REQUIRE(out2 || op != MOP_RETR_TRANSP, "sttode_manifold_rowop: retr_transp needs the out2 buffer");
    STT_REQUIRE(manifold != MF_POINCARE || (c > 0.f && finite_(c)), "sttode_manifold_rowop: curvature c must be positive and finite");
    const bool takes_w = op == MOP_PTRANSP || op == MOP_RETR_TRANSP || op == MOP_INNER;
    hipLaunchKernelGGL(manifold_row_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, op, manifold, a, b, takes_w ? w : nullptr, out,
                       out2, rows, d, (double)c);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_manifold_rowop_bwd(int op, int manifold, const float* a, const float* b, const float* w, const float* g, const float* g2,
                                         float* ga, float* gb, float* gw, int rows, int d, float c, void* stream) {
    STT_REQUIRE(op >= 0 && op < MOP_COUNT, "sttode_manifold_rowop_bwd: unknown op");
    STT_REQUIRE(manifold >= 0 && manifold < MF_COUNT, "sttode_manifold_rowop_bwd: unknown manifold");
    STT_REQUIRE(a && b, "sttode_manifold_rowop_bwd: null pointer");
    STT_REQUIRE(rows > 0 && d > 0, "sttode_manifold_rowop_bwd: empty shape");
    STT_REQUIRE(w || (op != MOP_PTRANSP && op != MOP_RETR_TRANSP), "sttode_manifold_rowop_bwd: this op needs the third operand");
    STT_REQUIRE(op == MOP_RETR_TRANSP ? (g || g2) : (g && !g2),
                "sttode_manifold_rowop_bwd: the upstream gradient g is required (retr_transp: g or g2, NULL meaning zero), g2 is retr_transp's alone");
    STT_REQUIRE(ga || gb || gw, "sttode_manifold_rowop_bwd: no gradient buffer given");
    STT_REQUIRE(manifold != MF_POINCARE || (c > 0.f && finite_(c)), "sttode_manifold_rowop_bwd: curvature c must be positive and finite");
    const bool takes_w = op == MOP_PTRANSP || op == MOP_RETR_TRANSP || op == MOP_INNER;
    hipLaunchKernelGGL(manifold_row_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, op, manifold, a, b, takes_w ? w : nullptr, g,
                       g2, ga, gb, takes_w ? gw : nullptr, rows, d, (double)c);
    STT_HIP(hipGetLastError());
    return 0;
}

extern "C" int sttode_riemannian_step(int rule, const void* table, int nrows_table, long total_slots, double lr, double beta1, double beta2,
                                      double eps, double weight_decay, double momentum, long t, void* tstate, void* stream) {
    STT_REQUIRE(rule >= 0 && rule < RULE_COUNT, "sttode_riemannian_step: unknown rule");
    STT_REQUIRE(table && nrows_table > 0 && total_slots > 0 && total_slots < (1L << 33), "sttode_riemannian_step: null table or no rows");
    STT_REQUIRE(finite_(lr) && lr >= 0. && finite_(weight_decay) && weight_decay >= 0., "sttode_riemannian_step: bad lr or weight_decay");
    const unsigned blocks = (unsigned)((total_slots + 3) / 4);
    hipStream_t s = (hipStream_t)stream;
    if (rule == RULE_ADAM) {
        STT_REQUIRE(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && finite_(eps) && eps >= 0., "sttode_riemannian_step: bad beta or eps");
        STT_REQUIRE(t >= 0 && (t >= 1 || tstate), "sttode_riemannian_step: the step count t must be >= 1, or 0 with a device count");
        if (t == 0) hipLaunchKernelGGL(riemannian_tick_kernel, dim3(1), dim3(1), 0, s, (double*)tstate);
        hipLaunchKernelGGL(riemannian_step_kernel<RULE_ADAM>, dim3(blocks), dim3(256), 0, s, (const RiemItem*)table, nrows_table, total_slots, lr,
                           beta1, beta2, eps, weight_decay, 0., (double)t, (double*)tstate);
    } else {
        STT_REQUIRE(finite_(momentum) && momentum >= 0., "sttode_riemannian_step: bad momentum");
        hipLaunchKernelGGL(riemannian_step_kernel<RULE_SGD>, dim3(blocks), dim3(256), 0, s, (const RiemItem*)table, nrows_table, total_slots, lr, 0.,
                           0., 0., weight_decay, momentum, 0., (double*)nullptr);
    }
    STT_HIP(hipGetLastError());
    return 0;
}
