// Multi-modal ground truth over a dataset: MMADE / MMFDE (include/sttode_hip.h sttode_multimodal).  For every agent i the
// agents j of its segment whose anchored history lies within eps of i's form its neighbour set; their futures, translated to i's anchor, are
// the futures that "similar histories actually had", and the K samples of i are scored by the mean over them of the best sample's distance.
//   mm_prepass_kernel   one thread per agent: the anchor and the anchored history vector as doubles into the caller's workspace, component-major
//                       [2 + 2h][n], so that a wave testing 64 consecutive j reads 512 contiguous bytes per component.
//   mm_main_kernel      one wave per agent i, four agents per workgroup: the lanes test j = j0 + lane over i's segment in tiles of 64; a ballot
//                       gives the tile's matches; per match, in ascending j, lane k computes its sample's distances to the translated future and
//                       a fixed xor tree of fmin gives the two minima, added to float64 running sums in j order.
// No LDS, no barriers, no atomics: runs give the same bits, and an agent's result depends on nothing outside its own segment.
#include <cfloat>
#include <cmath>

#include "api_util.hpp"
#include "set_body.hpp"
#include "../../include/sttode_hip.h"

namespace {

constexpr int MM_CH = 8;   // history components between two looks at the wave-wide early exit (their loads are issued together)
constexpr int MM_FT = 4;   // frames of a neighbour's future whose loads are issued together

// ws[0][i], ws[1][i]: the anchor a_i = P_i[Tp-1]; ws[2 + c][i], c = 2 (t - (Tp-1-h)) + {0: x, 1: y}: H_i = P_i[t] - a_i for t = Tp-1-h .. Tp-2.
// Coordinates are (double)(x * scale), the product in fp32.
__global__ __launch_bounds__(256) void mm_prepass_kernel(const float* __restrict__ past, int n, int Tp, int h, float scale,
                                                         double* __restrict__ ws) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float2* p = reinterpret_cast<const float2*>(past + (size_t)i * Tp * 2);
    const float2 a = p[Tp - 1];
    const double ax = (double)(a.x * scale), ay = (double)(a.y * scale);
    ws[i] = ax;
    ws[(size_t)n + i] = ay;
    for (int f = 0; f < h; ++f) {
        const float2 v = p[Tp - 1 - h + f];
        ws[(size_t)(2 + 2 * f) * n + i] = (double)(v.x * scale) - ax;
        ws[(size_t)(3 + 2 * f) * n + i] = (double)(v.y * scale) - ay;
    }
}

// Agent i = 4 blockIdx.x + wave.  Its segment [a0, a1) is found by a binary search of seg_ptr (every bound clamped to [0, n]; an agent that no
// segment of a malformed device seg_ptr covers keeps only itself), or is [0, n).  Lane l of tile j0 sums (H_i[c] - H_j[c])^2 over c in order
// for j = j0 + l (component c of agent j at the uniform address of the component plus a 32-bit lane offset);
// every MM_CH components the wave leaves the tile if no lane can still match (its partial sum is above thr, or NaN).  The decision is
// sqrt(sum) <= eps on the full sum.  lo < eps^2 < thr bracket eps^2 by 2^-40 relative (sttode_multimodal): a sum <= lo has a square root <= eps
// and one above thr has not, whatever the rounding, so the square root is taken only when some lane's sum lies between them, and neither the
// bracket nor the early exit ever changes a decision.  j == i always matches.
// Per match j (ascending): g[t] = (Y_j[t] - a_j) + a_i, lane k < K sums |X_i,k,t - g[t]| over the frames in order (the neighbour's frame and
// anchors are wave-uniform reads, the sample row comes from L1), a NaN result counts as +inf, and the xor tree's minima are added to the sums.
__global__ __launch_bounds__(256) void mm_main_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                      const int* __restrict__ seg_ptr, int S, int n, int K, int Tf, int h, float scale, double eps,
                                                      double lo, double thr, const double* __restrict__ ws, int* __restrict__ count, double* __restrict__ mmade,
                                                      double* __restrict__ mmfde) {
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (i >= n) return;
    int a0 = 0, a1 = n;
    if (seg_ptr) {
        int s0 = 0, s1 = S;
        while (s1 - s0 > 1) {
            const int mid = (s0 + s1) >> 1;
            if (seg_ptr[mid] <= i)
                s0 = mid;
            else
                s1 = mid;
        }
        clamped_segment(seg_ptr, s0, n, a0, a1);
        if (i < a0 || i >= a1) {
            a0 = i;
            a1 = i + 1;
        }
    }
    const int C = 2 * h;
    const char* __restrict__ H = reinterpret_cast<const char*>(ws + (size_t)2 * n);   // component c of agent a: H + c * cs + 8 a
    const size_t cs = (size_t)n * sizeof(double);
    const unsigned ioff = (unsigned)i * 8u;
    const double aix = ws[i], aiy = ws[(size_t)n + i];
    const float2* __restrict__ xk = reinterpret_cast<const float2*>(pred) + ((size_t)i * K + min(lane, K - 1)) * Tf;
    double sa = 0.0, sf = 0.0;
    int cnt = 0;
    for (int j0 = a0; j0 < a1; j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < a1;
        const unsigned joff = (unsigned)(valid ? j : a1 - 1) * 8u;
        double s = 0.0;
        int c0 = 0;
        for (; c0 + MM_CH <= C; c0 += MM_CH) {
            double hj[MM_CH], hi[MM_CH];
            const char* __restrict__ Hc = H + (size_t)c0 * cs;
#pragma unroll
            for (int c = 0; c < MM_CH; ++c) {
                hj[c] = *reinterpret_cast<const double*>(Hc + c * cs + joff);
                hi[c] = *reinterpret_cast<const double*>(Hc + c * cs + ioff);
            }
#pragma unroll
            for (int c = 0; c < MM_CH; ++c) {
                const double d = hi[c] - hj[c];
                s += d * d;
            }
            if (__ballot(valid && s <= thr) == 0) break;
        }
        if (c0 + MM_CH > C)   // (not left early: the last, short chunk)
            for (int c = c0; c < C; ++c) {
                const double d = *reinterpret_cast<const double*>(H + c * cs + ioff) - *reinterpret_cast<const double*>(H + c * cs + joff);
                s += d * d;
            }
        bool match = s <= lo;
        const bool near = !match && s <= thr;
        if (__ballot(valid && near) != 0) match = match || (near && sqrt(s) <= eps);
        unsigned long long m = __ballot(valid && (match || j == i));
        while (m) {
            const int jn = j0 + __builtin_ctzll(m);
            m &= m - 1;
            const float2* __restrict__ y = reinterpret_cast<const float2*>(gt) + (size_t)jn * Tf;
            const double ajx = ws[jn], ajy = ws[(size_t)n + jn];
            double sum = 0.0, dl = 0.0;
            int t = 0;
            for (; t + MM_FT <= Tf; t += MM_FT) {
                float2 v[MM_FT], r[MM_FT];
#pragma unroll
                for (int u = 0; u < MM_FT; ++u) {
                    v[u] = xk[t + u];
                    r[u] = y[t + u];
                }
#pragma unroll
                for (int u = 0; u < MM_FT; ++u) {
                    const double gx = ((double)(r[u].x * scale) - ajx) + aix, gy = ((double)(r[u].y * scale) - ajy) + aiy;
                    const double dx = (double)(v[u].x * scale) - gx, dy = (double)(v[u].y * scale) - gy;
                    dl = sqrt(dx * dx + dy * dy);
                    sum += dl;
                }
            }
            for (; t < Tf; ++t) {
                const float2 v = xk[t], r = y[t];
                const double gx = ((double)(r.x * scale) - ajx) + aix, gy = ((double)(r.y * scale) - ajy) + aiy;
                const double dx = (double)(v.x * scale) - gx, dy = (double)(v.y * scale) - gy;
                dl = sqrt(dx * dx + dy * dy);
                sum += dl;
            }
            double va = sum / (double)Tf, vf = dl;
            if (lane >= K || va != va) va = INFINITY;
            if (lane >= K || vf != vf) vf = INFINITY;
            sa += wave_min(va);
            sf += wave_min(vf);
            ++cnt;
        }
    }
    if (lane == 0) {
        count[i] = cnt;
        mmade[i] = sa / (double)cnt;
        mmfde[i] = sf / (double)cnt;
    }
}

}  // namespace

extern "C" int sttode_multimodal(const float* pred, const float* past, const float* gt, const int* seg_ptr, int n_seg, int n, int K, int Tp,
                                 int Tf, int hist_frames, float scale, double eps, double* ws, long ws_doubles, int* count, double* mmade,
                                 double* mmfde, void* stream) {
    const char* why = nullptr;
    if (!(pred && past && gt && ws && count && mmade && mmfde))
        why = "null pointer (pred, past, gt, ws, count, mmade and mmfde are required)";
    else if (n < 1 || n > (1 << 20))
        why = "needs 1 <= n <= 2^20 agents";
    else if (K < 1 || K > 64)
        why = "needs 1 <= K <= 64 (one lane per sample)";
    else if (Tf < 1)
        why = "Tf must be positive";
    else if (Tp < 2)
        why = "needs Tp >= 2 (an anchor and one history frame)";
    else if (hist_frames < 1 || hist_frames > Tp - 1)
        why = "needs 1 <= hist_frames <= Tp - 1";
    else if (!(eps >= 0.0) || std::isinf(eps))
        why = "eps must be non-negative and finite";
    else if (!std::isfinite(scale))
        why = "scale must be finite";
    else if (ws_doubles < (2L * hist_frames + 2L) * (long)n)
        why = "workspace too small: needs (2 hist_frames + 2) n doubles";
    else if (seg_ptr ? n_seg < 1 : n_seg != 0)
        why = "seg_ptr must be a CSR [n_seg + 1] with n_seg >= 1 (or NULL with n_seg = 0)";
    if (why) return stt_refuse("sttode_multimodal", why);
    hipLaunchKernelGGL(mm_prepass_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, past, n, Tp, hist_frames, scale, ws);
    STT_HIP(hipGetLastError());
    // lo < eps^2 < thr with room for every rounding of eps * eps, of the bounds and of a square root.  Where eps^2 overflows, every finite
    // sum has a square root <= eps; where it comes close to underflow, the bracket is left open and the square root decides alone.
    const double e2 = eps * eps;
    double lo = fmin(e2 * (1.0 - 0x1p-40), DBL_MAX), thr = e2 * (1.0 + 0x1p-40);
    if (eps > 0.0 && e2 < 0x1p-900) {
        lo = -1.0;
        thr = INFINITY;
    }
    hipLaunchKernelGGL(mm_main_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, pred, gt, seg_ptr, n_seg, n, K, Tf, hist_frames,
                       scale, eps, lo, thr, ws, count, mmade, mmfde);
    STT_HIP(hipGetLastError());
    return 0;
}
