// Oversample and reduce: Lloyd k-means of an agent's M sampled futures to K representatives (include/sttode_hip.h sttode_reduce_samples,
// DESIGN.md §4n).  One workgroup of 256 lanes per agent; labels, counts and centroids live in LDS across all iterations.
//   staging   the agent's samples (all frames) are copied once into LDS as xs[f][m] (row = coordinate f of 2 Tf, MP = M | 1 floats apart, so the
//             staging writes of consecutive f land on different banks and the reads of consecutive m are consecutive words) when they fit
//             beside the fixed arrays in 160 KiB; otherwise every pass reads them from global memory / L2 (the STAGED = false instantiation:
//             same operations on the same values in the same order, so the two forms give the same bits).
//   init      'first': samples 0 .. K-1; 'maximin': sample 0, then K-1 workgroup-wide argmax reductions over the running minimum distance
//             (lowest index on ties); caller's: init [n,K,Tf,2].
//   assign    lane -> SB samples (m = tid + 256 s) x 4 centroids per pass: the centroids are kept as ct[f][KP] (k contiguous, KP = K rounded
//             up to 4), so one 16-byte broadcast read serves four distances.  d(m, k) = sum over f >= 2 from_frame, in order, of
//             fma(x - c, x - c, d): direct differences, never the expanded form.  Strict < over ascending k: the lowest k wins exact ties.
//   update    a stable counting sort of the samples by label (sort_by_label of set_body.hpp: per 64-sample chunk one ballot per k gives each sample its rank among the
//             chunk's members of its cluster; a prefix over chunks and clusters gives the offsets), then one lane per (k, f) adds its
//             cluster's members IN SAMPLE ORDER and divides by the count; an empty cluster keeps its centroid.
//   stop      an iteration that changes no label would reproduce the same centroids: the loop ends there.
// No floating-point atomics, no cross-workgroup traffic: an agent's result depends on its own samples only.
#include "api_util.hpp"
#include "set_body.hpp"
#include "../../include/sttode_hip.h"

namespace {

struct Shape {
    int n, R, K_in, Tf, K, M, F, f0, KP, MP, chunks;
};

// LDS layout in bytes (every block 16-byte aligned): ct | xs (staged only) | cnt | off | red | lab | scratch | ccnt
struct Layout {
    int ct, xs, cnt, off, red, lab, scratch, ccnt, total;
};

__host__ __device__ inline Layout layout_of(const Shape& s, bool staged) {
    Layout l;
    int p = 0;
    l.ct = p;      p += up16(s.F * s.KP * 4);
    l.xs = p;      p += staged ? up16(s.F * s.MP * 4) : 0;
    l.cnt = p;     p += MAX_K * 4;
    l.off = p;     p += MAX_K * 4;
    l.red = p;     p += 64;
    l.lab = p;     p += up16(s.M);
    l.scratch = p; p += up16(4 * s.M);                    // maximin: float mind[M]; iterations: unsigned short rnk[M], perm[M]
    l.ccnt = p;    p += up16(s.chunks * s.KP * 2);        // per (64-sample chunk, cluster): member count, then exclusive prefix over chunks
    l.total = p;
    return l;
}

// A sample's coordinates: staged, a column of xs; streamed, its row of pred ([R,n,K_in,Tf,2]: sample m = r K_in + k).
template <bool STAGED>
struct Samples {
    const float* xs;
    const float* pred;
    int MP, n, K_in, F, a;
    __device__ __forceinline__ size_t row(int m) const { return STAGED ? (size_t)m : round_major_row(a, m, n, K_in, F); }
    __device__ __forceinline__ float at(size_t row, int f) const { return STAGED ? xs[(size_t)f * MP + row] : pred[row + f]; }
};

template <bool STAGED, int SB>
__global__ __launch_bounds__(NT) void reduce_kernel(const float* __restrict__ pred, Shape s, int iters, int init_mode,
                                                    const float* __restrict__ init, float* __restrict__ centroids, int* __restrict__ labels,
                                                    int* __restrict__ counts) {
    extern __shared__ __align__(16) unsigned char lds[];
    const Layout L = layout_of(s, STAGED);
    float* ct = reinterpret_cast<float*>(lds + L.ct);
    float* xs = reinterpret_cast<float*>(lds + L.xs);
    int* cnt = reinterpret_cast<int*>(lds + L.cnt);
    int* off = reinterpret_cast<int*>(lds + L.off);
    float* redv = reinterpret_cast<float*>(lds + L.red);
    int* redi = reinterpret_cast<int*>(lds + L.red + 32);
    unsigned char* lab = lds + L.lab;
    float* mind = reinterpret_cast<float*>(lds + L.scratch);
    unsigned short* rnk = reinterpret_cast<unsigned short*>(lds + L.scratch);
    unsigned short* perm = rnk + s.M;
    unsigned short* ccnt = reinterpret_cast<unsigned short*>(lds + L.ccnt);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = blockIdx.x;
    const int M = s.M, K = s.K, F = s.F, KP = s.KP, f0 = s.f0;
    const Samples<STAGED> X{xs, pred, s.MP, s.n, s.K_in, F, a};

    if (STAGED) {
        const int per = s.K_in * F;                                     // one round's samples of this agent are contiguous
        for (int r = 0; r < s.R; ++r) {
            const float* src = pred + ((size_t)r * s.n + a) * (size_t)per;
            for (int e = tid; e < per; e += NT) {
                const int k = e / F, f = e - k * F;
                xs[f * s.MP + r * s.K_in + k] = src[e];
            }
        }
    }
    for (int m = tid; m < M; m += NT) lab[m] = 255;
    if (tid < MAX_K) cnt[tid] = 0;
    for (int e = tid; e < F * (KP - K); e += NT) {                      // padding clusters K .. KP-1: finite, never chosen
        const int f = e / (KP - K), k = K + e - f * (KP - K);
        ct[f * KP + k] = 0.f;
    }
    __syncthreads();

    // ---- initial centroids ----
    if (init_mode == 2) {
        const float* src = init + (size_t)a * K * F;
        for (int e = tid; e < K * F; e += NT) {
            const int k = e / F, f = e - k * F;
            ct[f * KP + k] = src[e];
        }
    } else if (init_mode == 0) {
        for (int e = tid; e < K * F; e += NT) {
            const int k = e / F, f = e - k * F;
            ct[f * KP + k] = X.at(X.row(k), f);
        }
    } else {
        int chosen = 0;
        for (int j = 0; j < K; ++j) {
            // the chosen sample becomes centroid j; every sample's running minimum takes its distance to it
            const size_t crow = X.row(chosen);
            for (int f = tid; f < F; f += NT) ct[f * KP + j] = X.at(crow, f);
            if (j == K - 1) break;
            float bv = -1.f;
            int bi = 0;
            for (int m = tid; m < M; m += NT) {
                const size_t row = X.row(m);
                float d = 0.f;
                for (int f = f0; f < F; ++f) {
                    const float df = X.at(row, f) - X.at(crow, f);
                    d = __builtin_fmaf(df, df, d);
                }
                if (j > 0) d = d < mind[m] ? d : mind[m];
                mind[m] = d;
                take_higher(bv, bi, d, m);
            }
            wave_take_higher(bv, bi);
            __syncthreads();                                            // (the previous round's redv / redi have been read)
            if (lane == 0) {
                redv[wave] = bv;
                redi[wave] = bi;
            }
            __syncthreads();
            bv = redv[0];
            bi = redi[0];
            for (int w = 1; w < NT / 64; ++w) take_higher(bv, bi, redv[w], redi[w]);
            chosen = bi;
        }
    }
    __syncthreads();

    // ---- Lloyd iterations ----
    for (int it = 0; it < iters; ++it) {
        int changed = 0;
        for (int m0 = tid; m0 < M; m0 += NT * SB) {
            size_t row[SB];
            bool ok[SB];
            float best[SB];
            int bk[SB];
#pragma unroll
            for (int q = 0; q < SB; ++q) {
                ok[q] = m0 + NT * q < M;
                row[q] = X.row(ok[q] ? m0 + NT * q : m0);
                best[q] = __builtin_inff();
                bk[q] = 0;
            }
            for (int k0 = 0; k0 < KP; k0 += 4) {
                float acc[SB][4];
#pragma unroll
                for (int q = 0; q < SB; ++q)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[q][j] = 0.f;
                for (int f = f0; f < F; ++f) {
                    const float4 c4 = *reinterpret_cast<const float4*>(&ct[f * KP + k0]);
                    const float c[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                    for (int q = 0; q < SB; ++q) {
                        const float x = X.at(row[q], f);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float df = x - c[j];
                            acc[q][j] = __builtin_fmaf(df, df, acc[q][j]);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int q = 0; q < SB; ++q)
                        if (k0 + j < K && acc[q][j] < best[q]) {
                            best[q] = acc[q][j];
                            bk[q] = k0 + j;
                        }
            }
#pragma unroll
            for (int q = 0; q < SB; ++q)
                if (ok[q]) {
                    const int m = m0 + NT * q;
                    changed |= lab[m] != bk[q];
                    lab[m] = (unsigned char)bk[q];
                }
        }
        if (!__syncthreads_or(changed)) break;

        sort_by_label(lab, M, K, KP, s.chunks, rnk, ccnt, cnt, off);
        for (int m = tid; m < M; m += NT) perm[sorted_slot(m, lab, KP, rnk, ccnt, off)] = (unsigned short)m;
        __syncthreads();
        for (int p = tid; p < K * F; p += NT) {
            const int k = p / F, f = p - k * F;
            const int c = cnt[k];
            if (c == 0) continue;                                       // an empty cluster keeps its centroid
            const unsigned short* mem = perm + off[k];
            float sum = X.at(X.row(mem[0]), f);                         // (starting from the first member, not from +0: a lone -0 stays -0)
            for (int i = 1; i < c; ++i) sum += X.at(X.row(mem[i]), f);
            ct[f * KP + k] = sum / (float)c;
        }
        __syncthreads();
    }

    // ---- outputs (the loop leaves through its break or its last barrier: LDS is settled either way) ----
    for (int m = tid; m < M; m += NT) labels[(size_t)a * M + m] = lab[m];
    if (tid < K) counts[(size_t)a * K + tid] = cnt[tid];
    float* out = centroids + (size_t)a * K * F;
    for (int p = tid; p < K * F; p += NT) {
        const int k = p / F, f = p - k * F;
        out[p] = ct[f * KP + k];
    }
}

template <bool STAGED, int SB>
int launch(const float* pred, const Shape& s, int iters, int init_mode, const float* init, float* centroids, int* labels, int* counts,
           int bytes, hipStream_t st) {
    STT_SET_LDS_ONCE((reduce_kernel<STAGED, SB>), LDS_LIMIT);
    hipLaunchKernelGGL((reduce_kernel<STAGED, SB>), dim3((unsigned)s.n), dim3(NT), (size_t)bytes, st, pred, s, iters, init_mode, init,
                       centroids, labels, counts);
    STT_HIP(hipGetLastError());
    return 0;
}

template <bool STAGED>
int launch_sb(const float* pred, const Shape& s, int iters, int init_mode, const float* init, float* centroids, int* labels, int* counts,
              int bytes, hipStream_t st) {
    if (s.M <= NT) return launch<STAGED, 1>(pred, s, iters, init_mode, init, centroids, labels, counts, bytes, st);
    if (s.M <= 2 * NT) return launch<STAGED, 2>(pred, s, iters, init_mode, init, centroids, labels, counts, bytes, st);
    return launch<STAGED, 4>(pred, s, iters, init_mode, init, centroids, labels, counts, bytes, st);
}

}  // namespace

extern "C" int sttode_reduce_samples(const float* pred, int n, int R, int K_in, int Tf, int K, int iters, int from_frame, int init_mode,
                                     const float* init, float* centroids, int* labels, int* counts, void* stream) {
    STT_REQUIRE(pred && centroids && labels && counts, "sttode_reduce_samples: null pointer");
    STT_REQUIRE(n >= 1, "sttode_reduce_samples: n must be >= 1");
    STT_REQUIRE(K >= 1 && K <= MAX_K, "sttode_reduce_samples: K must be in [1, 64]");
    STT_REQUIRE(R >= 1 && K_in >= 1 && (long)R * K_in <= MAX_M && (long)R * K_in >= K,
                "sttode_reduce_samples: M = R K_in must be in [K, 4096]");
    STT_REQUIRE(Tf >= 1 && Tf <= MAX_TF, "sttode_reduce_samples: Tf must be in [1, 200]");
    STT_REQUIRE(from_frame >= 0 && from_frame < Tf, "sttode_reduce_samples: from_frame must be in [0, Tf)");
    STT_REQUIRE(iters >= 1 && iters <= MAX_ITERS, "sttode_reduce_samples: iters must be in [1, 1000]");
    STT_REQUIRE(init_mode >= 0 && init_mode <= 2, "sttode_reduce_samples: init_mode must be 0 (first), 1 (maximin) or 2 (caller's init)");
    STT_REQUIRE((init != nullptr) == (init_mode == 2), "sttode_reduce_samples: init must be given in init_mode 2 and only there");
    Shape s;
    s.n = n, s.R = R, s.K_in = K_in, s.Tf = Tf, s.K = K;
    s.M = R * K_in;
    s.F = 2 * Tf;
    s.f0 = 2 * from_frame;
    s.KP = (K + 3) & ~3;
    s.MP = s.M | 1;
    s.chunks = (s.M + 63) / 64;
    const bool staged = layout_of(s, true).total <= LDS_LIMIT;
    const int bytes = layout_of(s, staged).total;
    STT_REQUIRE(bytes <= LDS_LIMIT, "sttode_reduce_samples: internal: the fixed arrays exceed the LDS limit");
    hipStream_t st = (hipStream_t)stream;
    return staged ? launch_sb<true>(pred, s, iters, init_mode, init, centroids, labels, counts, bytes, st)
                  : launch_sb<false>(pred, s, iters, init_mode, init, centroids, labels, counts, bytes, st);
}
