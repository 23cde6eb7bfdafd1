// Oversample and reduce whole scenes: Lloyd k-means in which a sample is one future of a whole segment -- a scene, an NBA game -- so all
// agents of a segment share one label per sample and one count per cluster (include/sttode_hip.h sttode_reduce_scenes).
// One workgroup of 256 lanes per segment for the whole loop: no traffic between workgroups, and the early stop stays local.
//   centroids live in the OUTPUT array in global memory (a segment of hundreds of agents has hundreds of KiB of them); the workgroup's own
//             barriers order its stores and loads of them.  Labels, counts and the sort's arrays live in LDS across all iterations.
//   samples   are read from global memory (a segment's do not fit LDS): a lane reads its sample's slice of an agent in chunks of FC = 24
//             floats, the chunk's 16-byte loads issued together, so a 96-byte row of Tf = 12 is one visit to its cache lines per pass.
//   init      'first': scene futures 0 .. K-1; 'maximin': scene future 0, then K-1 workgroup-wide argmax reductions over the running minimum
//             of the float64 scene distance (lowest index on ties); caller's: init [n,K,Tf,2].
//   assign    lane -> SB samples (m = tid + 256 q) x KC = 4 KQ centroids per pass, cluster groups outermost, the segment's agents inside (K <= 20
//             is ONE pass: the samples are read once per iteration): up to AB agents' groups are staged through LDS as ctq[agent][f][KC], so one
//             16-byte broadcast read serves four distances.  Per agent d_a(m, k) = sum over f >= 2 from_frame, in order, of
//             fma(x - c, x - c, d) in fp32 -- the bits of reduce_kernel (reduce.hip) -- and D(m, k) += (double)d_a(m, k) in segment order in
//             SB x KC float64 registers.  Strict < over ascending k: the lowest k wins exact ties.
//   update    ONE stable counting sort of the samples by label per iteration (sort_by_label of set_body.hpp, as reduce_kernel: per 64-sample chunk one ballot per k, a prefix
//             over chunks and clusters), which leaves the members' row offsets in cluster order; then one lane per (agent, k, f), f fastest,
//             adds its cluster's members IN SAMPLE ORDER and divides by the count; an empty cluster's centroid is not touched.
//   stop      an iteration that changes no label would reproduce the same centroids: the loop ends there.
// No floating-point atomics, no workspace: a segment's result depends on its own agents' samples only.
#include "api_util.hpp"
#include "set_body.hpp"
#include "../../include/sttode_hip.h"

namespace {

constexpr int FC = 24;                        // floats of a sample's row held in registers at a time
constexpr int MAX_AB = 16, CTQ_BYTES = 32 * 1024;   // agents staged per barrier pair: as many groups [F][KC] as fit in CTQ_BYTES, at most MAX_AB

struct Shape {
    int n, R, K_in, Tf, K, M, F, f0, KP, AB, chunks, S;
};

// LDS layout in bytes (every block 16-byte aligned): ctq | cnt | off | red | lab | wide | rnk | ccnt
struct Layout {
    int ctq, cnt, off, red, lab, wide, rnk, ccnt, total;
};

__host__ __device__ inline Layout layout_of(const Shape& s, int KC) {
    Layout l;
    int p = 0;
    l.ctq = p;   p += up16(s.AB * s.F * KC * 4);
    l.cnt = p;   p += MAX_K * 4;
    l.off = p;   p += MAX_K * 4;
    l.red = p;   p += 64;                                   // double redv[4] | int redi[4]
    l.lab = p;   p += up16(s.M);
    l.wide = p;  p += up16(8 * s.M);                        // maximin: double mind[M]; iterations: size_t prow[M], the members' rows in cluster order
    l.rnk = p;   p += up16(2 * s.M);
    l.ccnt = p;  p += up16(s.chunks * s.KP * 2);            // per (64-sample chunk, cluster): member count, then exclusive prefix over chunks
    l.total = p;
    return l;
}

// p[0 .. cnt) into x (cnt even, <= FC; the rest of x is zero and never used) in 16- and 8-byte loads issued together.  A row starts at an even
// number of floats from pred, which itself need only be aligned as a float: the vector types carry that alignment.
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ void load_chunk(const float* p, int cnt, float (&x)[FC]) {
#pragma unroll
    for (int j = 0; j < FC; j += 4) {
        f4u v = {0.f, 0.f, 0.f, 0.f};                                   // (every element is written: the array stays in registers)
        if (j + 4 <= cnt) {
            v = *reinterpret_cast<const f4u*>(p + j);
        } else if (j + 2 <= cnt) {
            const f2u h = *reinterpret_cast<const f2u*>(p + j);
            v.x = h.x, v.y = h.y;
        }
        x[j] = v.x, x[j + 1] = v.y, x[j + 2] = v.z, x[j + 3] = v.w;
    }
}

template <int SB, int KQ>
__global__ __launch_bounds__(NT) void reduce_scenes_kernel(const float* __restrict__ pred, Shape s, int iters, int init_mode, const float* init,
                                                           const int* __restrict__ seg_ptr, float* centroids, int* __restrict__ labels,
                                                           int* __restrict__ counts) {
    constexpr int KC = 4 * KQ;                                          // centroids per pass
    extern __shared__ __align__(16) unsigned char lds[];
    const Layout L = layout_of(s, KC);
    float* ctq = reinterpret_cast<float*>(lds + L.ctq);
    int* cnt = reinterpret_cast<int*>(lds + L.cnt);
    int* off = reinterpret_cast<int*>(lds + L.off);
    double* redv = reinterpret_cast<double*>(lds + L.red);
    int* redi = reinterpret_cast<int*>(lds + L.red + 32);
    unsigned char* lab = lds + L.lab;
    double* mind = reinterpret_cast<double*>(lds + L.wide);
    size_t* prow = reinterpret_cast<size_t*>(lds + L.wide);
    unsigned short* rnk = reinterpret_cast<unsigned short*>(lds + L.rnk);
    unsigned short* ccnt = reinterpret_cast<unsigned short*>(lds + L.ccnt);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sg = blockIdx.x;
    const int M = s.M, K = s.K, F = s.F, KP = s.KP, f0 = s.f0, KF = s.K * s.F;
    int a0, a1;                                                         // clamped: a CSR on the device is never read back by the host
    clamped_segment(seg_ptr, sg, s.n, a0, a1);
    const int A = a1 - a0;
    int* lab_out = labels + (size_t)sg * M;
    int* cnt_out = counts + (size_t)sg * K;
    if (A == 0) {                                                       // an empty segment: every distance is 0, the lowest k wins
        for (int m = tid; m < M; m += NT) lab_out[m] = 0;
        if (tid < K) cnt_out[tid] = tid == 0 ? M : 0;
        return;
    }
    // sample m of agent a starts at row0(m) + a astr in pred ([R,n,K_in,Tf,2]: sample m = r K_in + k)
    const size_t astr = (size_t)s.K_in * F;
    auto row0 = [&](int m) -> size_t { return round_major_row(0, m, s.n, s.K_in, F); };
    float* cseg = centroids + (size_t)a0 * KF;                          // the segment's centroids [A][K][F]
    const float* xseg = pred + (size_t)a0 * astr;                       // the segment's samples: agent i of it at xseg + i astr

    for (int m = tid; m < M; m += NT) lab[m] = 255;
    if (tid < MAX_K) cnt[tid] = 0;

    // ---- initial centroids ----
    if (init_mode == 2) {
        const float* src = init + (size_t)a0 * KF;
        for (size_t e = tid; e < (size_t)A * KF; e += NT) cseg[e] = src[e];
    } else if (init_mode == 0) {
        for (size_t e = tid; e < (size_t)A * KF; e += NT) {
            const int i = (int)(e / KF), rem = (int)(e - (size_t)i * KF), k = rem / F, f = rem - k * F;
            cseg[e] = xseg[row0(k) + i * astr + f];
        }
    } else {
        int chosen = 0;
        for (int j = 0; j < K; ++j) {
            // the chosen scene future becomes centroid j of every agent; every sample's running minimum takes its distance to it
            const size_t crow = row0(chosen);
            for (int e = tid; e < A * F; e += NT) {
                const int i = e / F, f = e - i * F;
                cseg[((size_t)i * K + j) * F + f] = xseg[crow + i * astr + f];
            }
            if (j == K - 1) break;
            double bv = -1.0;
            int bi = 0;
            for (int m = tid; m < M; m += NT) {
                const size_t row = row0(m);
                double D = 0.0;
                for (int i = 0; i < A; ++i) {
                    const float* xa = xseg + i * astr;
                    float d = 0.f;
                    for (int fc = f0; fc < F; fc += FC) {
                        const int nf = F - fc < FC ? F - fc : FC;
                        float x[FC], c[FC];
                        load_chunk(xa + row + fc, nf, x);
                        load_chunk(xa + crow + fc, nf, c);
#pragma unroll
                        for (int f = 0; f < FC; ++f)
                            if (f < nf) {
                                const float df = x[f] - c[f];
                                d = __builtin_fmaf(df, df, d);
                            }
                    }
                    D += (double)d;
                }
                if (j > 0) D = D < mind[m] ? D : mind[m];
                mind[m] = D;
                take_higher(bv, bi, D, m);
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
    const int Fs = F - f0;
    for (int it = 0; it < iters; ++it) {
        int changed = 0;
        for (int mb = 0; mb < M; mb += NT * SB) {                       // (uniform trip counts: the staging below has barriers)
            const int m0 = mb + tid;
            size_t row[SB];
            bool ok[SB];
            double best[SB];
            int bk[SB];
#pragma unroll
            for (int q = 0; q < SB; ++q) {
                ok[q] = m0 + NT * q < M;
                row[q] = row0(ok[q] ? m0 + NT * q : 0);
                best[q] = (double)__builtin_inff();
                bk[q] = 0;
            }
            for (int k0 = 0; k0 < KP; k0 += KC) {
                double D[SB][KC];
#pragma unroll
                for (int q = 0; q < SB; ++q)
#pragma unroll
                    for (int j = 0; j < KC; ++j) D[q][j] = 0.0;
                for (int ab = 0; ab < A; ab += s.AB) {
                    const int nb = A - ab < s.AB ? A - ab : s.AB;
                    __syncthreads();                                    // the previous batch's groups have been read
                    for (int e = tid; e < nb * KC * Fs; e += NT) {      // clusters k0 .. k0+KC-1 of nb agents; clusters >= K: finite, never chosen
                        const int i = e / (KC * Fs), rem = e - i * KC * Fs, j = rem / Fs, f = f0 + rem - j * Fs;
                        ctq[(i * F + f) * KC + j] = k0 + j < K ? cseg[((size_t)(ab + i) * K + k0 + j) * F + f] : 0.f;
                    }
                    __syncthreads();
                    for (int i = 0; i < nb; ++i) {
                        const float* xa = xseg + (size_t)(ab + i) * astr;
                        const float* cq = ctq + i * F * KC;
                        float acc[SB][KC];
#pragma unroll
                        for (int q = 0; q < SB; ++q)
#pragma unroll
                            for (int j = 0; j < KC; ++j) acc[q][j] = 0.f;
                        for (int fc = f0; fc < F; fc += FC) {
                            const int nf = F - fc < FC ? F - fc : FC;
                            float x[SB][FC];
#pragma unroll
                            for (int q = 0; q < SB; ++q) load_chunk(xa + row[q] + fc, nf, x[q]);
#pragma unroll
                            for (int f = 0; f < FC; ++f) {
                                if (f < nf) {
#pragma unroll
                                    for (int g = 0; g < KQ; ++g) {
                                        const float4 c4 = *reinterpret_cast<const float4*>(&cq[(fc + f) * KC + 4 * g]);
                                        const float c[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                                        for (int q = 0; q < SB; ++q)
#pragma unroll
                                            for (int j = 0; j < 4; ++j) {
                                                const float df = x[q][f] - c[j];
                                                acc[q][4 * g + j] = __builtin_fmaf(df, df, acc[q][4 * g + j]);
                                            }
                                    }
                                }
                            }
                        }
#pragma unroll
                        for (int q = 0; q < SB; ++q)
#pragma unroll
                            for (int j = 0; j < KC; ++j) D[q][j] += (double)acc[q][j];
                    }
                }
#pragma unroll
                for (int j = 0; j < KC; ++j)
#pragma unroll
                    for (int q = 0; q < SB; ++q)
                        if (k0 + j < K && D[q][j] < best[q]) {
                            best[q] = D[q][j];
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
        for (int m = tid; m < M; m += NT) prow[sorted_slot(m, lab, KP, rnk, ccnt, off)] = row0(m);
        __syncthreads();
        for (size_t e = tid; e < (size_t)A * KF; e += NT) {
            const int i = (int)(e / KF), rem = (int)(e - (size_t)i * KF), k = rem / F, f = rem - k * F;
            const int c = cnt[k];
            if (c == 0) continue;                                       // an empty cluster keeps its centroid, for every agent alike
            const size_t* mem = prow + off[k];
            const float* xa = xseg + i * astr + f;
            float sum = xa[mem[0]];                                     // (starting from the first member, not from +0: a lone -0 stays -0)
            int p = 1;
            for (; p + 4 <= c; p += 4) {                                // (four loads in flight; the additions stay in member order)
                const float v0 = xa[mem[p]], v1 = xa[mem[p + 1]], v2 = xa[mem[p + 2]], v3 = xa[mem[p + 3]];
                sum += v0;
                sum += v1;
                sum += v2;
                sum += v3;
            }
            for (; p < c; ++p) sum += xa[mem[p]];
            cseg[e] = sum / (float)c;
        }
        __syncthreads();                                                // the stores are ordered in front of the next iteration's loads
    }

    // ---- outputs (the loop leaves through its break or its last barrier: LDS is settled either way) ----
    for (int m = tid; m < M; m += NT) lab_out[m] = lab[m];
    if (tid < K) cnt_out[tid] = cnt[tid];
}

template <int SB, int KQ>
int launch(const float* pred, Shape s, int iters, int init_mode, const float* init, const int* seg_ptr, float* centroids, int* labels,
           int* counts, hipStream_t st) {
    const int per_agent = s.F * 4 * KQ * 4;                             // bytes of one agent's staged group [F][KC]
    s.AB = CTQ_BYTES / per_agent < 1 ? 1 : (CTQ_BYTES / per_agent > MAX_AB ? MAX_AB : CTQ_BYTES / per_agent);
    const int bytes = layout_of(s, 4 * KQ).total;
    STT_REQUIRE(bytes <= LDS_LIMIT, "sttode_reduce_scenes: internal: the fixed arrays exceed the LDS limit");
    STT_SET_LDS_ONCE((reduce_scenes_kernel<SB, KQ>), LDS_LIMIT);
    hipLaunchKernelGGL((reduce_scenes_kernel<SB, KQ>), dim3((unsigned)s.S), dim3(NT), (size_t)bytes, st, pred, s, iters, init_mode, init, seg_ptr,
                       centroids, labels, counts);
    STT_HIP(hipGetLastError());
    return 0;
}

// centroids per pass: all of K <= 4, K <= 12 or K <= 20 in one; 20 per pass beyond
template <int SB>
int launch_kq(const float* pred, const Shape& s, int iters, int init_mode, const float* init, const int* seg_ptr, float* centroids, int* labels,
              int* counts, hipStream_t st) {
    if (s.K <= 4) return launch<SB, 1>(pred, s, iters, init_mode, init, seg_ptr, centroids, labels, counts, st);
    if (s.K <= 12) return launch<SB, 3>(pred, s, iters, init_mode, init, seg_ptr, centroids, labels, counts, st);
    return launch<SB, 5>(pred, s, iters, init_mode, init, seg_ptr, centroids, labels, counts, st);
}

}  // namespace

extern "C" int sttode_reduce_scenes(const float* pred, int n, int R, int K_in, int Tf, int K, int iters, int from_frame, int init_mode,
                                    const float* init, const int* seg_ptr, int S, float* centroids, int* labels, int* counts, void* stream) {
    STT_REQUIRE(pred && seg_ptr && centroids && labels && counts, "sttode_reduce_scenes: null pointer");
    STT_REQUIRE(n >= 1, "sttode_reduce_scenes: n must be >= 1");
    STT_REQUIRE(S >= 1, "sttode_reduce_scenes: S must be >= 1");
    STT_REQUIRE(K >= 1 && K <= MAX_K, "sttode_reduce_scenes: K must be in [1, 64]");
    STT_REQUIRE(R >= 1 && K_in >= 1 && (long)R * K_in <= MAX_M && (long)R * K_in >= K,
                "sttode_reduce_scenes: M = R K_in must be in [K, 4096]");
    STT_REQUIRE(Tf >= 1 && Tf <= MAX_TF, "sttode_reduce_scenes: Tf must be in [1, 200]");
    STT_REQUIRE(from_frame >= 0 && from_frame < Tf, "sttode_reduce_scenes: from_frame must be in [0, Tf)");
    STT_REQUIRE(iters >= 1 && iters <= MAX_ITERS, "sttode_reduce_scenes: iters must be in [1, 1000]");
    STT_REQUIRE(init_mode >= 0 && init_mode <= 2, "sttode_reduce_scenes: init_mode must be 0 (first), 1 (maximin) or 2 (caller's init)");
    STT_REQUIRE((init != nullptr) == (init_mode == 2), "sttode_reduce_scenes: init must be given in init_mode 2 and only there");
    Shape s;
    s.n = n, s.R = R, s.K_in = K_in, s.Tf = Tf, s.K = K, s.S = S;
    s.M = R * K_in;
    s.F = 2 * Tf;
    s.f0 = 2 * from_frame;
    s.KP = (K + 3) & ~3;
    s.AB = 1;                                                           // (set per instantiation: launch)
    s.chunks = (s.M + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    if (s.M <= NT) return launch_kq<1>(pred, s, iters, init_mode, init, seg_ptr, centroids, labels, counts, st);
    return launch_kq<2>(pred, s, iters, init_mode, init, seg_ptr, centroids, labels, counts, st);
}
