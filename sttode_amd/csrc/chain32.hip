// Fused per-trajectory decoder chain (round 2): ONE persistent kernel runs, for a group of 128 trajectories,
//     decoder_x MLP (block 0) -> d = x_true - x_hat0 -> decoder_y MLP (block 0) -> conv + GRU (block 1)
//     -> decoder_y MLP (block 1) -> pred = ((y_hat0 + y_hat1) + cur) + orig
// (model/STTODE.py:51-77 DecomposeBlock.forward x2, :320-347 Decoder.forward, :621-622), with every intermediate
// (d, state, the 512/256-wide hidden activations) in REGISTERS.  Round 1 ran this as three kernels (mlp_block0 ->
// gru_cols -> mlp_block1, csrc/decoder.hip) that exchanged dbuf / ybuf / state1 through HBM and each paid a grid tail.
//
// CDNA4 design:
//   * v_mfma_f32_32x32x2_f32: a wave owns 32 trajectories ("columns") on the 32 MFMA columns, features in registers.
//     One 32-feature x 32-column tile is a f32x16 per lane:  lane l: column l & 31, half h = l >> 5;
//     register j  <->  feature 8*(j/4) + 4*h + (j%4).  That accumulator layout IS the B-operand layout of the next
//     layer (MFMA step j consumes k-pair (8*(j/4) + j%4, +4)), so the whole chain needs no transpose and no LDS round trip.
//     Versus the 16x16x4 chain of round 1: half the MFMA instructions and half the A-operand LDS bytes per FLOP, no
//     dependent-accumulator stall (64-cycle issue = 64-cycle latency); measured 143.6 vs 135.2 TFLOP/s in the
//     weight-stream probe (profiles/r02/diag_probe.json).
//   * ALL weights (both MLPs of block 0, conv + GRU of block 1, the MLP of block 1: 3.2 MB per group) stream L2 -> LDS
//     by LDS-DMA (global_load_lds_dwordx4) in chunks of <= 3 "PK32" tiles of 4 KiB (tile = A operand of 16 MFMAs:
//     32 rows x 32 k), double buffered, one workgroup barrier per chunk; the chunk order is a host-built PROGRAM
//     (packing.chain_stream), so the kernel only consumes tiles in order.  The GRU's recurrent weights are streamed per
//     step like everything else (66 FLOP per streamed byte, the same intensity as the MLP layers), which frees the
//     144 KiB of LDS round 1 pinned for them: LDS per workgroup is 24 KiB ring + 32 KiB gather / z slots + 8 KiB biases.
//     Between a chunk's barrier and its first MFMA a wave issues the ring's first fragment reads and the DMA instructions, nothing else:
//     program entries are fetched in the middle of a step, addresses are made in front of the barrier, the tile count of the next chunk
//     is a constant of the call site wherever it is known, M0 is written once per pair of pieces and never restored (ChainStreamT).
//   * workgroup = 4 waves x 32 columns = 128 trajectories, 2 workgroups per CU (<= 256 VGPRs per wave); groups are
//     handed out by an atomic work counter (one tail for the whole chain instead of three, and a later launch on
//     another stream fills it: the kernel holds no chip-wide resource).
#include "chain.hpp"
#include "latency_bodies.hpp"
#include "frontend_body.hpp"
#include "api_util.hpp"
#include "../../include/sttode_hip.h"
#include <cstdlib>
#include <cstddef>

// C32_DIAG_TRACE (diagnostic build, profiles/exp_r03_trace.py): every workgroup appends one record {launch tag, block, kind, start, end (100 MHz
// s_memrealtime), HW_ID, XCC_ID} to the debug buffer -- who ran where and when, across overlapping launches
#ifdef C32_DIAG_TRACE
__shared__ long long g_tr_ph[4];   // role phase stamps (thread 0)
#define C32_TRACE_BEGIN() long long _tr_t0 = 0, _tr_c0 = 0; if (threadIdx.x == 0 && A.dbg) { _tr_t0 = __builtin_amdgcn_s_memrealtime(); _tr_c0 = __builtin_amdgcn_s_memtime(); }
#define C32_TRACE_END(kind) do { if (threadIdx.x == 0 && A.dbg) { \
        const long long _t1 = __builtin_amdgcn_s_memrealtime(); unsigned _hw, _xcc; \
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(_hw)); asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(_xcc)); \
        const unsigned long long _r = atomicAdd((unsigned long long*)A.dbg, 1ull); if ((long long)_r >= A.dbg[1]) break; /* dbg[1] = capacity in records */ \
        long long* _p = A.dbg + 8 + _r * 12; _p[0] = A.trace_tag; _p[1] = blockIdx.x; _p[2] = (kind); _p[3] = _tr_t0; _p[4] = _t1; _p[5] = _hw; _p[6] = _xcc; \
        _p[8] = g_tr_ph[0]; _p[9] = g_tr_ph[1]; _p[10] = g_tr_ph[2]; _p[7] = __builtin_amdgcn_s_memtime() - _tr_c0; _p[11] = g_tr_ph[3]; } } while (0)
#define C32_TRACE_PHASE(i) do { if (threadIdx.x == 0) g_tr_ph[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define C32_TRACE_PHASE(i) do { } while (0)
#define C32_TRACE_BEGIN() do { } while (0)
#define C32_TRACE_END(kind) do { } while (0)
#endif

#include "role_body.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// diagnostic builds (profiles/exp_chain_variants.sh; never shipped): -DC32_DIAG_NODMA / _NOGATHER / _NOBARRIER / _NOGATES
// (timing ablations), -DC32_DIAG_STAMPS (stamps, also of the chunk steps), -DC32_DIAG_CHECK (a static tile count that is not the program's traps)
#ifdef C32_DIAG_NOGATES
#define C32_SIG(x) ((x) * 1e-3f)
#define C32_TANH(x) ((x) * 1e-3f)
#else
#define C32_SIG(x) sigmoid_prescaled(x)
#define C32_TANH(x) tanh_prescaled(x)
#endif

#define C32_TILE 256                        // f32x4 per tile (4 KiB)
#define C32_CMAX 3                          // tiles per chunk
#define C32_RING (2 * C32_CMAX * C32_TILE)  // f32x4 in the double buffer (24 KiB)
#define C32_SLOT 256                        // f32x4 per wave gather slot (4 KiB)

struct Role32Args {   // throughput-form per-agent roles (role32.hpp)
    const f32x4* pool; const int2* prog; int prog_len; const float* consts;   // packing.role_stream (the host picks the variant)
    const float* enc_in; const int* last;                                     // [n][4 Tp] encoder inputs, [n] last-agent flag (scenes variant)
    const float* g_in; const float* attn; int ld_attn;                        // NBA variant: g [n][64], attention output before out_proj; attn == nullptr: scenes
    const float* xpad; int ldx;                                               // [n][ldx] normalised track, flattened (t, c), zero padded
    float* pf; float* state0; float* A0x; float* A0y; float* A1y;             // [n][128], [n][96], [n][512] x 3
    int n, Tp, kte, nwg;                                                      // agents, observed frames, k-tiles of x, role workgroups in the grid
    float ode_time;
    int prio;       // > 0: the role waves run at s_setprio 3 (stt_chain_lagged sets 3)
    int* counter;   // work queue of THIS call's trajectory groups (a later launch of the same stream): zeroed by role workgroup 0
    float* zgen; unsigned zkey0, zkey1; int K;   // zgen != nullptr: the roles draw this call's latents z [n K][32] ~ N(0, I) themselves (role32.hpp latents32)
    // past != nullptr (scene batches): the roles run STTODENet.set_data for their own 128 agents first (role32.hpp frontend32) -- no front-end
    // launch.  past / scene_ptr may be device memory or pinned host memory (the reads then ARE the H2D transfer of the call's inputs).
    const float* past; const int* scene_ptr; int S; float* scene_orig; int* agent_scene;
    float* enc_in_w; float* xpad_w; float* cur_w; float* orig_w; int* last_w;
    float* m_ade; float* m_fde;   // fused metrics of this call (ChainArgs::m_*): set to +inf here, atomicMin'ed by its groups two launches later
};

struct ChainArgs {
    const float* A0x; const float* A0y; const float* A1y;  // [nagents][512] per-agent layer-1 pre-activations (b1 included)
    const f32x4* pool;                                      // PK32 tile pool
    const int2* prog; int prog_len;                         // chunk program of ONE group: (first tile, tiles <= 3)
    const float* consts;                                    // biases, layout below
    const float* z;                                         // [ncols][32]
    const float* xpad; int ldx;                             // [nagents][ldx] normalised past, flattened (t,c), zero padded
    const float* cur; const float* orig;                    // [nagents][2]
    float* pred;                                            // [ncols][Tf2]; WRITE-ONLY for the kernel when `park` is another buffer (may then be pinned host memory)
    float* park;                                            // [ncols][Tf2] where block 0's y_hat0 waits for the epilogue (== pred: the round-2/3 layout)
    int* counter;                                           // work queue (zeroed before the launch)
    int ncols, K, Tp, Tf2;
    int persistent;  // 1: workgroups pull groups from the work queue until it is empty; 0: one group per workgroup (grid = groups)
    // fused metrics (lagged launch, optional): min-over-K ADE / FDE of the predictions against gt [nagents][Tf][2] (utils/metrics.py:7-26) by
    // the groups themselves -- each column's two values in best_of_k_kernel's summation order, then atomicMin on the float bits (>= 0)
    // into ade / fde [nagents], which the roles of the same call set to +inf two launches earlier
    const float* m_gt; float* m_ade; float* m_fde; float m_scale;
    int nworkers;    // lagged launch with workers: worker w starts with group w, further groups are tickets nworkers + counter++
    long long* dbg;  // diagnostic builds only (C32_DIAG_STAMPS / C32_DIAG_TRACE): per-workgroup stamps
    int trace_tag;   // diagnostic builds only: launch number
    int xcd_map;     // fused launch, roles in front: group blocks b, b + 8, b + 16, .. (dispatched to ONE XCD) take consecutive group ids
    RoleArgs R;      // fused launch only (traj_chain_kernel<NY, 1>)
    Role32Args R32;  // lagged launch only (traj_chain_kernel<NY, 2>): throughput-form roles of ANOTHER call in front of this call's groups
};

// consts layout (floats): b2x[256] b3x[32] | b2y[256] b3y[32*NY] | gbias[4][96] convb[32] | b2m[256] b3m[32*NY]
template <int NY> struct C32Const {
    static constexpr int b2x = 0, b3x = 256, b2y = 288, b3y = 544, gb = 544 + 32 * NY, cb = gb + 384, b2m = cb + 32,
                         b3m = b2m + 256, total = b3m + 32 * NY;
};

__device__ __forceinline__ f32x16 splat16(float v) {
    f32x16 r;
#pragma unroll
    for (int e = 0; e < 16; ++e) r[e] = v;
    return r;
}
__device__ __forceinline__ f32x16 relu16(f32x16 v) {
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = fmaxf(v[e], 0.f);
    return v;
}
// 32 consecutive features starting at p (LDS or global), in accumulator layout: register 4a+b <- p[8a + 4h + b]
__device__ __forceinline__ f32x16 ldrows(const float* p, int h) {
    f32x16 r;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const f32x4 v = ld4(p + 8 * a + 4 * h);
        r[4 * a + 0] = v[0]; r[4 * a + 1] = v[1]; r[4 * a + 2] = v[2]; r[4 * a + 3] = v[3];
    }
    return r;
}

// The chunk program in global memory, read with scalar loads (s_load_dwordx2: the entries arrive in SGPRs, no LDS copy, no readfirstlane).
typedef const __attribute__((address_space(4))) int KProg;   // (first, count) pairs as flat ints

// BUF: f32x4 per ring buffer (= the largest chunk).  GEN = false: program entries are (first PK32 tile, tiles <= 3) of 4-KiB tiles;
// GEN = true (exploratory bf16-split mode: tiles of 6 and 4 KiB in one pool): (offset in f32x4 units, number of 1-KiB pieces).
// Every address of the DMA is uniform but the lane's 16 B: the source advances in SGPRs (glds16_sv), the lane offset is one VGPR.
//
// A chunk step is  begin() .. MFMAs .. end().  What a wave issues between the barrier in end() and the first MFMA behind it is serial, un-hidden
// issue time once per 48 MFMAs, so the step keeps that stretch to the ring's first fragment reads and the DMA instructions themselves:
//   * fetch(): the program entry of the chunk after next is loaded in the MIDDLE of a step (tile_mma2f: halfway through the step's first
//     tile), never behind the barrier: scalar loads and LDS reads share lgkmcnt and scalar loads return out of order, so a scalar load in
//     flight turns every fragment wait into lgkmcnt(0) and exposes its full latency.  A step without MFMAs in front of its end() has its
//     entry fetched one step early (fetch_more / take_prefetched); a step that fetched nothing loads in end(), in front of the barrier.
//   * end(): everything the next begin() needs -- pool addresses (64-bit), the
//     M0 values of the ring destination, the piece count -- is computed IN FRONT of the barrier, where it is free for every wave but the
//     last to arrive, and carried in SGPRs.
//   * begin(N): the next chunk's tile count as a constant argument wherever the call site knows it: N DMA instructions in a straight
//     line, no compare / branch per piece.  begin() is the run-time form (TileFeed, phase ends, GEN).  A wave's pieces i = 0, 1, 2 are
//     4 096 B apart in the pool and in the ring: pieces 2k and 2k + 1 share one scalar base and one M0 write (glds16_m0).
//
// DYN: begin(N) ignores N and takes the program's count (traj_chain_kernel sets it for the two instantiations that the straight-line
// issue pushes into scratch).
template <int BUF, bool GEN, bool DYN = false>
struct ChainStreamT {
    static constexpr int kBuf = BUF;
    static constexpr int kPieces = (BUF / 64 + 3) / 4, kPairs = (kPieces + 1) / 2;   // 1-KiB pieces per wave of the largest chunk, and pairs of them
    const char* pool; KProg* prog; f32x4* ring;
    unsigned ring_addr, loff;  // loff: this lane's byte offset in a 1-KiB piece
    unsigned qoff, qend;       // byte offset in the program of the entry the next fetch loads; the program's size in bytes
    int par, lane, wave;
    int2 ld_v, ld_w;           // loaded entries: of the chunk after next (consumed by end()), and one more (fetch_more)
    bool fetched;              // this step has its entry (compile-time knowledge wherever the step is straight-line code)
    int cnt;                   // tiles of the chunk whose begin() comes next (TileFeed)
    // the DMA of the next begin(), made by end(): scalar base and M0 of piece pair k (both at the pair's second piece), pieces of this wave
    const char* nsrc[kPairs]; unsigned nm0[kPairs]; int ncnt, npc;
#ifdef C32_DIAG_STAMPS
    long long t_bar, gap_cyc, gap_n, gap_cal;   // barrier -> fragments landed and DMA issued, summed over the chunk steps (s_memtime)
#endif
    __device__ __forceinline__ int2 entry_at(unsigned off) const {
        const KProg* e = reinterpret_cast<const KProg*>(reinterpret_cast<const __attribute__((address_space(4))) char*>(prog) + off);
        return make_int2(e[0], e[1]);
    }
    __device__ __forceinline__ unsigned next_off(unsigned off) const { return off + 8 >= qend ? 0u : off + 8; }
    // addresses of chunk `ev` into ring buffer `buf`; the values are pinned where they are computed (hipcc would sink the arithmetic to its use)
    __device__ __forceinline__ void stage(int2 ev, int buf) {
        // (readfirstlane: a no-op where hipcc sees that the entry is uniform -- everywhere in the trajectory chain)
        ncnt = __builtin_amdgcn_readfirstlane(ev.y);
        npc = GEN ? (ncnt - wave + 3) >> 2 : ncnt;   // wave w moves pieces w, w + 4, w + 8, ... of 1 KiB; a PK32 tile is one piece per wave
        const size_t src = (size_t)(unsigned)__builtin_amdgcn_readfirstlane(ev.x) * (GEN ? 16u : C32_TILE * 16u) + (unsigned)wave * 1024u;   // 64-bit, as it always was
        const unsigned dst = __builtin_amdgcn_readfirstlane(ring_addr + (unsigned)buf * (BUF * 16) + (unsigned)wave * 1024u);
#pragma unroll
        for (int k = 0; k < kPairs; ++k) {
            nsrc[k] = pool + (src + 4096u * (2 * k + 1));
            nm0[k] = dst + 4096u * (2 * k + 1);
            asm volatile("" : "+s"(nsrc[k]), "+s"(nm0[k]));
        }
        asm volatile("" : "+s"(npc));
    }
    __device__ __forceinline__ void issue(int N) {   // N > 0 (a constant once inlined): that many pieces, unconditionally; N == 0: npc of them
#ifndef C32_DIAG_NODMA
#pragma unroll
        for (int k = 0; k < kPairs; ++k) {
            if (N > 0 ? 2 * k < N : 2 * k < npc) {
                glds16_sv<-4096>(nsrc[k], loff, nm0[k] - 4096u);   // (M0 = nm0[k])
                if (2 * k + 1 < kPieces && (N > 0 ? 2 * k + 1 < N : 2 * k + 1 < npc)) glds16_m0<0>(nsrc[k], loff);
            }
        }
#endif
    }
    __device__ __forceinline__ void init(const f32x4* pool_, const int2* prog_, int len_, f32x4* ring_) {
        pool = reinterpret_cast<const char*>(pool_); prog = (KProg*)prog_; ring = ring_;
        ring_addr = __builtin_amdgcn_readfirstlane(lds_addr(ring_));
        lane = threadIdx.x & 63;
        loff = (unsigned)lane * 16;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        par = 0;
        qend = (unsigned)len_ * 8u;
        const int2 e0 = entry_at(0);
        stage(e0, 0);
        issue(0);
        cnt = e0.y;
        qoff = next_off(0);
        stage(entry_at(qoff), 1);
        qoff = next_off(qoff);
        fetched = false;
#ifdef C32_DIAG_STAMPS
        gap_cyc = 0; gap_n = 0;
        const long long c0 = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        gap_cal = __builtin_amdgcn_s_memtime() - c0;   // an empty stamp pair
        t_bar = 0;
#endif
    }
    // the entry of the chunk after next: call once per chunk step between begin() and end(), with MFMAs on both sides
    __device__ __forceinline__ void fetch() { ld_v = entry_at(qoff); qoff = next_off(qoff); fetched = true; }
    // ... and the entry behind it, for a following step that has no MFMAs to fetch between; that step calls take_prefetched() instead
    __device__ __forceinline__ void fetch_more() { ld_w = entry_at(qoff); qoff = next_off(qoff); }
    __device__ __forceinline__ void take_prefetched() { ld_v = ld_w; fetched = true; }
    __device__ __forceinline__ void stamp_gap() {
#ifdef C32_DIAG_STAMPS
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const long long c1 = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (t_bar) { gap_cyc += c1 - t_bar; ++gap_n; }
#endif
    }
    // start of a chunk step: prefetch the next chunk into the other buffer (its readers passed the previous barrier).  N: its tiles, if the
    // call site knows them (a constant after inlining; GEN = false); 0: the program's count
    __device__ __forceinline__ void begin(int N = 0) {
        __builtin_amdgcn_sched_barrier(0);
#ifdef C32_DIAG_CHECK
        if (!GEN && N > 0 && ncnt != N) __builtin_trap();   // the call site's static tile count is not the program's
#endif
        cnt = ncnt;
        issue(GEN || DYN ? 0 : N);
        stamp_gap();
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ const f32x4* cur() const { return ring + par * BUF + lane; }
    // end of a chunk step: this wave's DMA pieces have landed (vmcnt), then everybody's (barrier).  has_entry: the caller knows that this
    // step fetched (TileFeed, whose control flow hipcc cannot follow)
    __device__ __forceinline__ void end(bool has_entry = false) {
        __builtin_amdgcn_sched_barrier(0);
#ifdef C32_DIAG_CHECK
        if (has_entry && !fetched) __builtin_trap();   // the caller's claim does not hold: this step fetched nothing
#endif
        if (!has_entry && !fetched) fetch();
        stage(ld_v, par);   // the chunk after next goes where this step's chunk is: its readers are done at the barrier below
        __builtin_amdgcn_sched_barrier(0);
#ifndef C32_DIAG_NOBARRIER
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#endif
#ifdef C32_DIAG_STAMPS
        t_bar = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (no scalar load in flight across the fragment reads; its latency is gap_cal)
#endif
        par ^= 1;
        fetched = false;
        __builtin_amdgcn_sched_barrier(0);
    }
};
typedef ChainStreamT<C32_CMAX * C32_TILE, false> ChainStream;

// acc += Atile (32 rows x 32 k, PK32) * B (32 k x 32 columns in accumulator layout)
__device__ __forceinline__ void tile_mma(f32x16& acc, const f32x4* __restrict__ t, const f32x16& B) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 a = t[g * 64];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r], B[4 * g + r], acc, 0, 0, 0);
    }
}

// The four 1-KiB LDS-DMA pieces of a 32-feature block of per-lane rows into a gather slot: lane (c, h) fetches features 8a + 4h .. + 3,
// a = 0..3, of the row at byte offset `voff` from the uniform `base` (voff includes the 16 h); the step of a folds into the immediate.
__device__ __forceinline__ void gather_rows(const void* base, unsigned voff, unsigned slot_addr) {
    glds16_sv<0>(base, voff, slot_addr);
    glds16_sv<32>(base, voff, slot_addr + 1024);
    glds16_sv<64>(base, voff, slot_addr + 2048);
    glds16_sv<96>(base, voff, slot_addr + 3072);
}
// lane's byte offset of row `row` (of `width` floats) in a gather table, the lane half's 16 B included
__device__ __forceinline__ unsigned row_off(int row, int width, int h) { return (unsigned)row * (unsigned)(width * 4) + (unsigned)h * 16; }

// Software-pipelined form.  A lone wave per SIMD issues in order: with the fragment reads placed right in front of their MFMAs
// (what hipcc does with tile_mma) every pair of reads costs ~40 idle matrix-pipe cycles (LDS latency ~100 vs the 64-cycle shadow of
// the previous MFMA), and the first reads of a chunk sit behind the DMA issue.  Here the fragments of a tile are registers handed
// in (`cur`), the next tile's fragments of the same chunk are requested halfway through this tile, and the first tile of a chunk is
// read BEFORE the chunk's DMA pieces are issued (ChainStream::begin), so its latency overlaps that issue.
struct Frag { f32x4 a[4]; };
__device__ __forceinline__ void ldfrag(Frag& f, const f32x4* __restrict__ t) {
#pragma unroll
    for (int g = 0; g < 4; ++g) f.a[g] = t[g * 64];
}
__device__ __forceinline__ void tile_mma2(f32x16& acc, const Frag& cur, const f32x16& B, Frag& nxt, const f32x4* __restrict__ tn) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (g == 2 && tn) {
            ldfrag(nxt, tn);
            __builtin_amdgcn_sched_barrier(0);   // hipcc otherwise sinks these reads back in front of their first use
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[g][r], B[4 * g + r], acc, 0, 0, 0);
    }
}

// tile_mma2 for the FIRST tile of a chunk step: halfway through it the stream fetches its program entries (nf: 1, or 2 with fetch_more).
template <class ST>
__device__ __forceinline__ void tile_mma2f(ST& st, f32x16& acc, const Frag& cur, const f32x16& B, Frag& nxt, const f32x4* __restrict__ tn, int nf = 1) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (g == 2) {
            __builtin_amdgcn_sched_barrier(0);   // the scalar load stays here: hoisted to the top of the step it would sit behind the barrier
            if (nf >= 1) st.fetch();
            if (nf >= 2) st.fetch_more();
            if (tn) ldfrag(nxt, tn);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[g][r], B[4 * g + r], acc, 0, 0, 0);
    }
}

// Layers 1+2 of one MLP for this wave's 32 columns: acc2 (256 rows = 8 tiles) += W2 relu(A0[agent] + W1v [z | Bh]).
// Per 32-row hidden tile: 1 + KH layer-1 tiles then 8 layer-2 tiles, a chunk boundary every 3 tiles ((1 + KH + 8) % 3 == 0).
// z (the first layer-1 k-tile's B operand) is read from the wave's LDS z slot every hidden tile (it would cost 16 VGPRs for the
// whole group otherwise; the kernel has 256 and must not spill: a kernel with ANY scratch pays a scratch set-up per dispatch).
// The per-agent pre-activation rows arrive through the wave's gather slot (4 x 16 B per lane per hidden tile, LDS-DMA):
// this lane's A0 row is at byte offset aoff of table tab; the row the NEXT phase starts with at aoff_next of tab_next.
template <int KH, class ST>
__device__ __forceinline__ void mlp_l12(ST& st, const f32x4* slot, const f32x4* zslot, const f32x16* Bh, const float* tab, unsigned aoff,
                                        const float* tab_next, unsigned aoff_next, f32x16 (&acc2)[8], int lane) {
    const unsigned slot_addr = __builtin_amdgcn_readfirstlane(lds_addr(slot));
    constexpr int KT1 = 1 + KH;
    static_assert((KT1 + 8) % 3 == 0, "hidden tile must be a whole number of chunks");
#pragma unroll
    for (int R = 0; R < 8; ++R) acc2[R] = splat16(0.f);
#pragma unroll 1
    for (int ht = 0; ht < 16; ++ht) {
        f32x16 h1, zb;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const f32x4 v = slot[a * 64 + lane];
            h1[4 * a + 0] = v[0]; h1[4 * a + 1] = v[1]; h1[4 * a + 2] = v[2]; h1[4 * a + 3] = v[3];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const f32x4 v = zslot[a * 64 + lane];
            zb[4 * a + 0] = v[0]; zb[4 * a + 1] = v[1]; zb[4 * a + 2] = v[2]; zb[4 * a + 3] = v[3];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slot is re-filled by the gather issued next
        __builtin_amdgcn_sched_barrier(0);
        const bool nl = ht + 1 < 16;   // (uniform) the next hidden tile's rows: the hidden-tile step advances the scalar base
        const void* nb = nl ? (const void*)(reinterpret_cast<const char*>(tab) + 128 * (ht + 1)) : (const void*)tab_next;
        const unsigned no = nl ? aoff : aoff_next;
        Frag fr[2];
#pragma unroll
        for (int i = 0; i < KT1 + 8; ++i) {
            if (i % 3 == 0) {
                if (i > 0) st.end();
                ldfrag(fr[i & 1], st.cur());       // first tile of the chunk: its read latency overlaps the DMA issue below
                st.begin(3);                       // the next chunk is one of this phase's or the first of layer 3: three tiles
                if (i == 0) {
#ifndef C32_DIAG_NOGATHER
                    gather_rows(nb, no, slot_addr);
#endif
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            const f32x4* tn = (i % 3 < 2) ? st.cur() + (i % 3 + 1) * C32_TILE : nullptr;
            if (i == 0) {
                tile_mma2f(st, h1, fr[i & 1], zb, fr[(i + 1) & 1], tn);
            } else if (i < KT1) {
                if (i % 3 == 0) tile_mma2f(st, h1, fr[i & 1], Bh[i - 1], fr[(i + 1) & 1], tn);
                else tile_mma2(h1, fr[i & 1], Bh[i - 1], fr[(i + 1) & 1], tn);
            } else {
                if (i == KT1) h1 = relu16(h1);
                if (i % 3 == 0) tile_mma2f(st, acc2[i - KT1], fr[i & 1], h1, fr[(i + 1) & 1], tn);
                else tile_mma2(acc2[i - KT1], fr[i & 1], h1, fr[(i + 1) & 1], tn);
            }
        }
        st.end();
    }
}

// Layer 3: out[o] = b3 + W3[o] relu(acc2 + b2), NO output tiles of 32 rows; 8 k-tiles per output tile, chunks of 3 tiles.
// NEXT: tiles of the chunk that follows the layer's last one (the next phase's first), if the caller knows them; 0: the program's count.
template <int NO, int NEXT = 0, class ST>
__device__ __forceinline__ void mlp_l3(ST& st, f32x16 (&acc2)[8], const float* __restrict__ b2, const float* __restrict__ b3,
                                       f32x16 (&out)[NO], int h) {
#pragma unroll
    for (int R = 0; R < 8; ++R) {
        STT_FENCE();  // keep the bias reads next to their use (hoisted as a block they spill)
        const f32x16 b = ldrows(b2 + 32 * R, h);
        acc2[R] = relu16(acc2[R] + b);
        asm volatile("" : "+v"(acc2[R]));  // ... and the add right behind its read (8 bias tiles in flight = 128 VGPRs otherwise)
    }
    STT_FENCE();
#pragma unroll
    for (int o = 0; o < NO; ++o) out[o] = ldrows(b3 + 32 * o, h);
    Frag fr[2];
#pragma unroll
    for (int i = 0; i < 8 * NO; ++i) {
        if (i % 3 == 0) {
            if (i > 0) st.end();
            ldfrag(fr[i & 1], st.cur());
            const int left = 8 * NO - (i + 3);   // tiles of this layer behind the chunk that starts here
            st.begin(left >= 3 ? 3 : left > 0 ? left : NEXT);
        }
        const f32x4* tn = (i % 3 < 2 && i + 1 < 8 * NO) ? st.cur() + (i % 3 + 1) * C32_TILE : nullptr;
        if (i % 3 == 0) tile_mma2f(st, out[i / 8], fr[i & 1], acc2[i % 8], fr[(i + 1) & 1], tn);
        else tile_mma2(out[i / 8], fr[i & 1], acc2[i % 8], fr[(i + 1) & 1], tn);
    }
    st.end();
}

// ---------------------------------------------------------------------------------------------------
// EXPLORATORY (round 3, opt-in, never the default): the two block-0 MLPs on the bf16 matrix cores with fp32-class accuracy.
// x = hi + mid + lo (three bf16 values, 8 mantissa bits each: 24 bits, what fp32 holds), W likewise (split on the host, packing.pk32b_tile);
// W x ~ lo.hi + hi.lo + mid.mid + mid.hi + hi.mid + hi.hi (the three dropped products are <= 2^-24 relative), fp32 accumulate:
// six v_mfma_f32_32x32x16_bf16 (32 cycles each) per 16-deep k block = 384 matrix-pipe cycles per 32 x 32 x 32 tile against 1 024 for
// sixteen 32x32x2 fp32 MFMAs.  The fp32 accumulator layout of a layer is still the B layout of the next: k slot s of lane half h of
// k block kb <-> accumulator register 8 kb + s.  Costs: the split of every activation tile (11 VALU instructions per pair of values),
// 1.5x the A-operand bytes.  Measured in the chain's weight-stream structure: 252 vs 143 fp32-equivalent TFLOP/s
// (profiles/r03/bf16x3_probe.json, csrc/diag/diag.hip shape 6).
// ---------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
#define C32_TILE_B3 384                     // f32x4 per bf16-split tile (6 KiB)
#define C32_BUF_B3 (C32_CMAX * C32_TILE_B3) // f32x4 per ring buffer in the exploratory mode (18 KiB)
struct B3 { bf16x8 p[3][2]; };              // [plane: hi, mid, lo][k block]
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ void split3(const f32x16& x, B3& o) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        unsigned hi[4], mi[4], lo[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float x0 = x[8 * kb + 2 * q], x1 = x[8 * kb + 2 * q + 1];
            const f32x2v v = {x0, x1};
            hi[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
            const float r0 = x0 - bf_lo(hi[q]), r1 = x1 - bf_hi(hi[q]);
            const f32x2v rv = {r0, r1};
            mi[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(rv, bf16x2));
            const f32x2v qv = {r0 - bf_lo(mi[q]), r1 - bf_hi(mi[q])};
            lo[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(qv, bf16x2));
        }
        const u32x4v H = {hi[0], hi[1], hi[2], hi[3]}, M = {mi[0], mi[1], mi[2], mi[3]}, L = {lo[0], lo[1], lo[2], lo[3]};
        o.p[0][kb] = __builtin_bit_cast(bf16x8, H);
        o.p[1][kb] = __builtin_bit_cast(bf16x8, M);
        o.p[2][kb] = __builtin_bit_cast(bf16x8, L);
    }
}
struct Frag6 { f32x4 a[6]; };               // [k block * 3 + plane]
__device__ __forceinline__ void ldfrag6(Frag6& f, const f32x4* __restrict__ t) {
#pragma unroll
    for (int i = 0; i < 6; ++i) f.a[i] = t[i * 64];
}
// acc += tile x B; the next tile's six fragments are requested halfway (tn != nullptr), like tile_mma2.  Small products first.
__device__ __forceinline__ void tile_mma_b3(f32x16& acc, const Frag6& cur, const B3& B, Frag6& nxt, const f32x4* __restrict__ tn) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        if (kb == 1 && tn) {
            ldfrag6(nxt, tn);
            __builtin_amdgcn_sched_barrier(0);
        }
        const bf16x8 ah = __builtin_bit_cast(bf16x8, cur.a[kb * 3 + 0]), am = __builtin_bit_cast(bf16x8, cur.a[kb * 3 + 1]),
                     al = __builtin_bit_cast(bf16x8, cur.a[kb * 3 + 2]);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, B.p[0][kb], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, B.p[2][kb], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, B.p[1][kb], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, B.p[0][kb], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, B.p[1][kb], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, B.p[0][kb], acc, 0, 0, 0);
    }
}
// acc += tile x B without look-ahead: the tile's six fragments are read here (the register-tight block-1 form; the SIMD's other wave
// covers the LDS latency)
__device__ __forceinline__ void tile_mma_b3n(f32x16& acc, const f32x4* __restrict__ t, const B3& B) {
    Frag6 f, dummy;
    ldfrag6(f, t);
    tile_mma_b3(acc, f, B, dummy, nullptr);
}
// mlp_l12<KH> on split tiles: per hidden tile 1 + KH layer-1 tiles (B = z, then the KH state tiles Bh: each split HERE from its fp32
// registers -- keeping three more tiles as planes would cost 72 VGPRs the kernel does not have) + 8 layer-2 row tiles.
// PRE: fragment look-ahead across tiles (KH = 0); without it 24 fewer VGPRs (KH = 3).
template <int KH, bool PRE, class ST>
__device__ __forceinline__ void mlp_l12_b3(ST& st, const f32x4* slot, const f32x4* zslot, const f32x16* Bh, const float* tab, unsigned aoff,
                                           const float* tab_next, unsigned aoff_next, f32x16 (&acc2)[8], int lane) {
    const unsigned slot_addr = __builtin_amdgcn_readfirstlane(lds_addr(slot));
    constexpr int KT1 = 1 + KH;
    static_assert((KT1 + 8) % 3 == 0, "hidden tile must be a whole number of chunks");
#pragma unroll
    for (int R = 0; R < 8; ++R) acc2[R] = splat16(0.f);
    // KH == 0 (block 0): z's planes are made ONCE per phase and stay in registers (24 VGPRs this form can afford: 16 splits and 64 LDS
    // reads fewer per phase); KH == 3 (block 1) has no registers to spare and re-splits z from its fp32 LDS slot per hidden tile
    B3 Bz;
    if (KH == 0) {
        f32x16 zb;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const f32x4 v = zslot[a * 64 + lane];
            zb[4 * a + 0] = v[0]; zb[4 * a + 1] = v[1]; zb[4 * a + 2] = v[2]; zb[4 * a + 3] = v[3];
        }
        split3(zb, Bz);
    }
#pragma unroll 1
    for (int ht = 0; ht < 16; ++ht) {
        f32x16 h1;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const f32x4 v = slot[a * 64 + lane];
            h1[4 * a + 0] = v[0]; h1[4 * a + 1] = v[1]; h1[4 * a + 2] = v[2]; h1[4 * a + 3] = v[3];
        }
        B3 Bt;
        if (KH == 0) {
            Bt = Bz;
        } else {
            f32x16 zb;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const f32x4 v = zslot[a * 64 + lane];
                zb[4 * a + 0] = v[0]; zb[4 * a + 1] = v[1]; zb[4 * a + 2] = v[2]; zb[4 * a + 3] = v[3];
            }
            split3(zb, Bt);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slot is re-filled by the gather issued next
        __builtin_amdgcn_sched_barrier(0);
        const bool nl = ht + 1 < 16;
        const void* nb = nl ? (const void*)(reinterpret_cast<const char*>(tab) + 128 * (ht + 1)) : (const void*)tab_next;
        const unsigned no = nl ? aoff : aoff_next;
        Frag6 fr[2];
#pragma unroll
        for (int i = 0; i < KT1 + 8; ++i) {
            if (i % 3 == 0) {
                if (i > 0) st.end();
                if (PRE) ldfrag6(fr[i & 1], st.cur());
                st.begin();
                if (i == 0) {
#ifndef C32_DIAG_NOGATHER
                    gather_rows(nb, no, slot_addr);
#endif
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            const f32x4* tc = st.cur() + (i % 3) * C32_TILE_B3;
            const f32x4* tn = (i % 3 < 2) ? tc + C32_TILE_B3 : nullptr;
            if (i > 0 && i < KT1) {
                STT_FENCE();
                split3(Bh[i - 1], Bt);                // state tile i-1 of this wave's columns
            }
            f32x16& acc = i < KT1 ? h1 : acc2[i < KT1 ? 0 : i - KT1];
            if (PRE) tile_mma_b3(acc, fr[i & 1], Bt, fr[(i + 1) & 1], tn);
            else tile_mma_b3n(acc, tc, Bt);
            if (i == KT1 - 1) {
                h1 = relu16(h1);
                split3(h1, Bt);                       // the hidden tile's planes take the registers of the layer-1 operand's
            }
        }
        st.end();
    }
}
// mlp_l3 on split tiles, k-tile major: activation tile T is split once and feeds all NO output tiles.
template <int NO, class ST>
__device__ __forceinline__ void mlp_l3_b3(ST& st, f32x16 (&acc2)[8], const float* __restrict__ b2, const float* __restrict__ b3,
                                          f32x16 (&out)[NO], int h) {
#pragma unroll
    for (int o = 0; o < NO; ++o) out[o] = ldrows(b3 + 32 * o, h);
    Frag6 fr[2];
    B3 Bt;
#pragma unroll
    for (int i = 0; i < 8 * NO; ++i) {
        if (i % NO == 0) {
            STT_FENCE();
            const f32x16 b = ldrows(b2 + 32 * (i / NO), h);
            const f32x16 a = relu16(acc2[i / NO] + b);
            split3(a, Bt);
        }
        if (i % 3 == 0) {
            if (i > 0) st.end();
            ldfrag6(fr[i & 1], st.cur());
            st.begin();
        }
        const f32x4* tn = (i % 3 < 2 && i + 1 < 8 * NO) ? st.cur() + (i % 3 + 1) * C32_TILE_B3 : nullptr;
        tile_mma_b3(out[i % NO], fr[i & 1], Bt, fr[(i + 1) & 1], tn);
    }
    st.end();
}

// planes -> fp32 (hi + mid + lo; within 2^-25 relative of the value that was split): the previous state for the GRU's blend
__device__ __forceinline__ f32x16 b3_to_f32(const B3& b) {
    f32x16 r;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        const u32x4v H = __builtin_bit_cast(u32x4v, b.p[0][kb]), M = __builtin_bit_cast(u32x4v, b.p[1][kb]), L = __builtin_bit_cast(u32x4v, b.p[2][kb]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            r[8 * kb + 2 * q] = (bf_lo(H[q]) + bf_lo(M[q])) + bf_lo(L[q]);
            r[8 * kb + 2 * q + 1] = (bf_hi(H[q]) + bf_hi(M[q])) + bf_hi(L[q]);
        }
    }
    return r;
}
// gru32_steps on split tiles (exploratory mode): the step's B operands -- conv input d (constant over the steps), conv output e, the
// three state tiles -- are split ONCE per step (each feeds 9 gate tiles); the new state is kept fp32 until the step ends, then split.
// Same tile order as the fp32 stream: per step 1 conv tile (a chunk of its own), then per j: r:[e h0 h1 h2] z:[e h0 h1 h2] n_h:[h0 h1 h2]
// n_i:[e] = 4 chunks of 3 tiles.  No fragment look-ahead (registers: 96 + 24 of planes, 48 of new state, up to 48 of gates).
template <class ST>
__device__ __forceinline__ void gru32_steps_b3(ST& st, const float* gb, const float* cb, const f32x16& d, f32x16 (&hs)[3], int Tp, int h) {
    B3 dB, hB[3];
    split3(d, dB);
#pragma unroll
    for (int j = 0; j < 3; ++j) split3(hs[j], hB[j]);
    constexpr int T = C32_TILE_B3;
#pragma unroll 1
    for (int t = 0; t < Tp; ++t) {
        B3 eB;
        {
            f32x16 e = ldrows(cb, h);
            st.begin();
            tile_mma_b3n(e, st.cur(), dB);
            e = relu16(e);
            st.end();
            split3(e, eB);
        }
        f32x16 hn[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            STT_FENCE();
            f32x16 ar = ldrows(gb + 0 * 96 + 32 * j, h);
            st.begin();
            tile_mma_b3n(ar, st.cur(), eB);
            tile_mma_b3n(ar, st.cur() + T, hB[0]);
            tile_mma_b3n(ar, st.cur() + 2 * T, hB[1]);
            st.end(); st.begin();
            tile_mma_b3n(ar, st.cur(), hB[2]);
#pragma unroll
            for (int r = 0; r < 16; ++r) ar[r] = C32_SIG(ar[r]);          // r gate
            STT_FENCE();
            f32x16 az = ldrows(gb + 1 * 96 + 32 * j, h);
            tile_mma_b3n(az, st.cur() + T, eB);
            tile_mma_b3n(az, st.cur() + 2 * T, hB[0]);
            st.end(); st.begin();
            tile_mma_b3n(az, st.cur(), hB[1]);
            tile_mma_b3n(az, st.cur() + T, hB[2]);
#pragma unroll
            for (int r = 0; r < 16; ++r) az[r] = C32_SIG(az[r]);          // z gate
            STT_FENCE();
            f32x16 an = ldrows(gb + 3 * 96 + 32 * j, h);
            tile_mma_b3n(an, st.cur() + 2 * T, hB[0]);
            st.end(); st.begin();
            tile_mma_b3n(an, st.cur(), hB[1]);
            tile_mma_b3n(an, st.cur() + T, hB[2]);
            {
                const f32x16 bi = ldrows(gb + 2 * 96 + 32 * j, h);
#pragma unroll
                for (int r = 0; r < 16; ++r) an[r] = fmaf(ar[r], an[r], bi[r]);     // b_in + r * (W_hn h + b_hn)
            }
            STT_FENCE();
            tile_mma_b3n(an, st.cur() + 2 * T, eB);                                 // + W_in e
            st.end();
            const f32x16 hp = b3_to_f32(hB[j]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float ng = C32_TANH(an[r]);
                hn[j][r] = fmaf(az[r], hp[r] - ng, ng);  // (1-z) n + z h
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            hs[j] = hn[j];
            split3(hn[j], hB[j]);
        }
    }
}

// conv tile of step t (a chunk of its own) + relu.  ZS: only the fragment groups g (k = 8g .. 8g+7) that meet the tile's non-zero
// columns 2t-2 .. 2t+3 (frames t-1 .. t+1, packing.toeplitz_conv) are read and multiplied: the others add exact zeros.
// The next chunk is a gate chunk of three tiles.  pre: the step in front fetched this step's program entry too (the conv chunk has at
// most 16 MFMAs to hide a scalar load behind); otherwise it is fetched behind the MFMAs.
template <bool ZS, class ST>
__device__ __forceinline__ f32x16 gru32_conv(ST& st, const float* cb, const f32x16& d, int t, int Tp, int h, bool pre) {
    f32x16 e = ldrows(cb, h);
    Frag fa, fb;
    if (ZS) {
        const int k0 = 2 * t - 2, k1 = 2 * t + 3;
        const int g0 = (k0 > 0 ? k0 : 0) >> 3, g1 = (k1 < 2 * Tp - 1 ? k1 : 2 * Tp - 1) >> 3;   // (uniform)
        const f32x4* tc = st.cur();
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (g >= g0 && g <= g1) fa.a[g] = tc[g * 64];
        st.begin(3);
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (g >= g0 && g <= g1)
#pragma unroll
                for (int r = 0; r < 4; ++r) e = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.a[g][r], d[4 * g + r], e, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (pre) st.take_prefetched();
        else st.fetch();
    } else {
        ldfrag(fa, st.cur());
        st.begin(3);
        tile_mma2f(st, e, fa, d, fb, nullptr, pre ? 0 : 1);
        if (pre) st.take_prefetched();
    }
    e = relu16(e);
    st.end();
    return e;
}

// conv1d(k=3) + relu + GRU(32 -> 96) over Tp steps for this wave's 32 columns, every weight tile streamed per step
// (model/STTODE.py:62-69; gate rows pre-scaled, chain.hpp): d = the flattened (t, c) input rows in accumulator layout, hs = h (in/out),
// gb = gate biases [4][96] (r, z, b_in, b_hn), cb = conv bias [32], both in LDS.  Per step: 1 conv tile (a chunk of its own) and 36
// gate tiles = 12 chunks.  Shared by the fused chain (block 1, per trajectory), gru32_kernel and the throughput-form roles (block 0, per agent).
// ZS (skip products known to be zero): the initial state is h = 0 (hs is not read) and step 0 issues no MFMA on it -- its 27 recurrent
// tiles are still consumed chunk by chunk, so the program is the same -- and the conv tiles issue only their non-zero fragment groups.
// A skipped product adds an exact zero: results are unchanged up to the sign of an exactly-zero value.  ZS = false: every tile in full
// (STTODE_GRU_ZERO_SKIP=0, A/B).
// Chunk steps (ChainStreamT): every chunk is followed by one of three tiles (begin(3)) but a step's last, which is followed by the next
// step's conv tile or by whatever comes after the GRU (begin(): the program's count).  Each step's first tile fetches the program entry
// (tile_mma2f); with ZS a step's last chunk fetches the following conv chunk's as well, and in step 0 the chunk in front of the one
// without MFMAs fetches for both.
template <bool ZS, class ST>
__device__ __forceinline__ void gru32_steps(ST& st, const float* gb, const float* cb, const f32x16& d, f32x16 (&hs)[3], int Tp, int h) {
    if (ZS) {   // step 0, h = 0: per j only the three e tiles; the third of the four chunks holds recurrent tiles alone
        const f32x16 e = gru32_conv<ZS>(st, cb, d, 0, Tp, h, false);
        Frag fa, fb;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            STT_FENCE();
            f32x16 ar = ldrows(gb + 0 * 96 + 32 * j, h);
            ldfrag(fa, st.cur()); st.begin(3);                          // [r:e h0 h1]
            tile_mma2f(st, ar, fa, e, fb, nullptr);
            st.end(); ldfrag(fa, st.cur() + 1 * C32_TILE); st.begin(3);  // [r:h2 z:e h0]
#pragma unroll
            for (int r = 0; r < 16; ++r) ar[r] = C32_SIG(ar[r]);
            STT_FENCE();
            f32x16 az = ldrows(gb + 1 * 96 + 32 * j, h);
            tile_mma2f(st, az, fa, e, fb, nullptr, 2);                   // (the entry of the next step too: it has no MFMAs)
            st.end(); st.begin(3);                                       // [z:h1 h2 n_h:h0]
            st.take_prefetched();
#pragma unroll
            for (int r = 0; r < 16; ++r) az[r] = C32_SIG(az[r]);
            STT_FENCE();
            f32x16 an = ldrows(gb + 3 * 96 + 32 * j, h);                  // W_hn h = 0
            {
                const f32x16 bi = ldrows(gb + 2 * 96 + 32 * j, h);
#pragma unroll
                for (int r = 0; r < 16; ++r) an[r] = fmaf(ar[r], an[r], bi[r]);     // b_in + r * (W_hn h + b_hn)
            }
            st.end(); ldfrag(fa, st.cur() + 2 * C32_TILE);               // [n_h:h1 h2 n_i:e]
            if (j < 2) st.begin(3); else st.begin();
            STT_FENCE();
            tile_mma2f(st, an, fa, e, fb, nullptr, (j == 2 && 1 < Tp) ? 2 : 1);   // + W_in e
            st.end();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float ng = C32_TANH(an[r]);
                hs[j][r] = fmaf(az[r], 0.f - ng, ng);   // (1-z) n + z h; the other tiles of hs are not read in step 0
            }
        }
    }
#pragma unroll 1
    for (int t = ZS ? 1 : 0; t < Tp; ++t) {
        const f32x16 e = gru32_conv<ZS>(st, cb, d, t, Tp, h, ZS);
        Frag fa, fb;
        f32x16 hn[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            // 12 tiles: r:[e h0 h1 h2] z:[e h0 h1 h2] n_h:[h0 h1 h2] n_i:[e]; chunk boundary every 3 tiles.
            // One gate accumulator is live at a time (finished gates shrink to their 16 outputs).
            STT_FENCE();
            f32x16 ar = ldrows(gb + 0 * 96 + 32 * j, h);
            ldfrag(fa, st.cur()); st.begin(3);
            tile_mma2f(st, ar, fa, e, fb, st.cur() + 1 * C32_TILE);
            tile_mma2(ar, fb, hs[0], fa, st.cur() + 2 * C32_TILE);
            tile_mma2(ar, fa, hs[1], fb, nullptr);
            st.end(); ldfrag(fa, st.cur()); st.begin(3);
            tile_mma2f(st, ar, fa, hs[2], fb, st.cur() + 1 * C32_TILE);
#pragma unroll
            for (int r = 0; r < 16; ++r) ar[r] = C32_SIG(ar[r]);          // r gate
            STT_FENCE();
            f32x16 az = ldrows(gb + 1 * 96 + 32 * j, h);
            tile_mma2(az, fb, e, fa, st.cur() + 2 * C32_TILE);
            tile_mma2(az, fa, hs[0], fb, nullptr);
            st.end(); ldfrag(fa, st.cur()); st.begin(3);
            tile_mma2f(st, az, fa, hs[1], fb, st.cur() + 1 * C32_TILE);
            tile_mma2(az, fb, hs[2], fa, st.cur() + 2 * C32_TILE);
#pragma unroll
            for (int r = 0; r < 16; ++r) az[r] = C32_SIG(az[r]);          // z gate
            STT_FENCE();
            f32x16 an = ldrows(gb + 3 * 96 + 32 * j, h);
            tile_mma2(an, fa, hs[0], fb, nullptr);
            st.end(); ldfrag(fa, st.cur());
            if (j < 2) st.begin(3); else st.begin();
            tile_mma2f(st, an, fa, hs[1], fb, st.cur() + 1 * C32_TILE, (ZS && j == 2 && t + 1 < Tp) ? 2 : 1);
            tile_mma2(an, fb, hs[2], fa, st.cur() + 2 * C32_TILE);
            {
                const f32x16 bi = ldrows(gb + 2 * 96 + 32 * j, h);
#pragma unroll
                for (int r = 0; r < 16; ++r) an[r] = fmaf(ar[r], an[r], bi[r]);     // b_in + r * (W_hn h + b_hn)
            }
            STT_FENCE();
            tile_mma2(an, fa, e, fb, nullptr);                                       // + W_in e
            st.end();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float ng = C32_TANH(an[r]);
                hn[j][r] = fmaf(az[r], hs[j][r] - ng, ng);  // (1-z) n + z h
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) hs[j] = hn[j];
    }

}

#include "role32.hpp"

// makes a per-lane integer opaque to the optimiser: address arithmetic derived from it is redone where it is used instead of
// being computed once at the top of the group and kept live (64-bit pointers held across phases were what spilled)
__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+v"(v)); return v; }

#ifdef C32_DIAG_STAMPS
#define C32_STAMP(k) do { if (threadIdx.x == 0 && A.dbg && gi < 4) { A.dbg[((size_t)blockIdx.x * 4 + gi) * 16 + 2 * (k)] = __builtin_amdgcn_s_memtime(); \
                                                                    A.dbg[((size_t)blockIdx.x * 4 + gi) * 16 + 2 * (k) + 1] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#else
#define C32_STAMP(k) do { } while (0)
#endif

// Grid order of the fused launch: blocks [0, ntiles) are the roles, one per 16-agent tile, and the trajectory groups follow.  Every role a
// group needs has a smaller block index: workgroups are dispatched in index order PER XCD (each XCD takes block % 8), and a role never
// waits, so within ONE launch every producer finishes whatever its consumers do (no deadlock; the bounded spin of wait_tiles is the
// backstop).  Several such launches in flight on different queues have no such guarantee across XCDs: the pipelined path uses the lagged
// form (FUSE = 2), which has no hand-off.  (Roles interleaved with the groups, and five role workgroups per tile, were tried and lost:
// DESIGN_HISTORY.md.)

// XCD-aware group order.  Workgroups are dealt to the 8 XCDs round-robin in dispatch order, and each XCD has its own L2.  A 16-agent tile's
// table rows (3 x 2 KiB per agent, written through to memory by its role) are read by the 2-3 trajectory groups of its 320 trajectories; in
// plain block order those are consecutive blocks = different XCDs, and every one of them fetches the rows from the fabric again.  With
// group id = (blocks of one XCD get a contiguous range) the sharers run behind the same L2.  A permutation of which block computes which
// group: results unchanged; producers (roles) still precede every group.
__host__ __device__ __forceinline__ int xcd_group(int b, int G) {
    const int x = b & 7, i = b >> 3, q = G >> 3, r = G & 7;
    return x * q + (x < r ? x : r) + i;
}

// FUSE: 0 = trajectory groups only; 1 = round-3 fused launch (latency-form roles of THIS call in front, tile flags); 2 = lagged launch
// (round 4: throughput-form roles of a LATER call in front, no dependency inside the launch; either part may be empty).
// ZS: the GRUs run as gru32_steps<ZS> (a template argument: a run-time choice inside the kernel costs the group path spills)
template <int NY, int FUSE, bool B3M, bool ZS>
__global__ __launch_bounds__(256, 2) void traj_chain_kernel(ChainArgs A) {
    // <1, 2, false, false> and <2, 1, false, true> keep the run-time piece count: with the straight-line issue hipcc spills two VGPRs in them
    // (12 B/lane of scratch that the parent form did not have); every other instantiation has the same or less scratch than before
    constexpr bool kDynCount = !B3M && ((NY == 1 && FUSE == 2 && !ZS) || (NY == 2 && FUSE == 1 && ZS));
    typedef ChainStreamT<B3M ? C32_BUF_B3 : C32_CMAX * C32_TILE, B3M, kDynCount> Stream;   // B3M: exploratory bf16-split mode (block-0 MLPs)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* ring = reinterpret_cast<f32x4*>(smem);
    f32x4* slots = ring + 2 * Stream::kBuf;
    f32x4* zslots = slots + 4 * C32_SLOT;
    float* cst = reinterpret_cast<float*>(zslots + 4 * C32_SLOT);
    int* sq = reinterpret_cast<int*>(cst + C32Const<NY>::total);  // [2]: this workgroup's first group / the group after the current one
    typedef C32Const<NY> CO;

    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const f32x4* slot = slots + wave * C32_SLOT;
    const f32x4* zslot = zslots + wave * C32_SLOT;
    const unsigned slot_addr = __builtin_amdgcn_readfirstlane(lds_addr(slot));
    const unsigned zslot_addr = __builtin_amdgcn_readfirstlane(lds_addr(zslot));
    const int ngroups = (A.ncols + 127) >> 7;

    C32_TRACE_BEGIN();
    if (FUSE == 2 && (int)blockIdx.x < A.R32.nwg) {   // (uniform) a throughput-form role workgroup: 128 agents of the roles' call
        role32_body<ZS>(*(KRole32Args*)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(ChainArgs, R32)),
                    blockIdx.x, smem);
        C32_TRACE_END(1);
        return;
    }
    // position among the group blocks; FUSE 1: < 0 for the roles in front, one workgroup per 16-agent tile.  (The role's tile is taken
    // from fb, behind the group order: with blockIdx.x, or with the role branch in front of the order, hipcc gives the NY = 2 and NY = 3
    // instantiations 32-36 B/lane more scratch -- profiles/fused_launch/resource_usage.txt)
    int fb = FUSE == 0 ? (int)blockIdx.x : (int)blockIdx.x - (FUSE == 2 ? A.R32.nwg : A.R.ntiles);
    if (FUSE && A.xcd_map && fb >= 0) fb = xcd_group(fb, ngroups);   // (roles in front: fb was the group block's position in dispatch order)
    if (FUSE == 1 && fb < 0) {   // (uniform) a per-agent role
        agent_role(A.R, (A.ncols + A.K - 1) / A.K, A.Tp, A.ldx, A.xpad, A.R.ntiles + fb, smem);
        C32_TRACE_END(1);
        return;
    }
    for (int i = threadIdx.x; i < CO::total; i += blockDim.x) cst[i] = A.consts[i];
    // A.persistent (FUSE 0 / 2): the workgroup is a WORKER that pulls groups from the call's work queue until it is empty.  Lagged launch:
    // worker w starts with group w and draws tickets only for its further groups, and not at all when every group has a worker --
    // same-address atomics of a whole grid starting together serialise at ~1 us each (measured: 213 workers, +0.2 ms per launch)
    if (threadIdx.x == 0) sq[0] = FUSE == 2 ? fb : (FUSE == 0 && A.persistent) ? atomicAdd(A.counter, 1) : FUSE ? fb : (int)blockIdx.x;
    if (FUSE == 1) {   // this group's per-agent tables come from role workgroups of THIS launch: wait for their tiles (one wave polls)
        const int g0 = fb;
        const int c_lo = g0 * 128, c_hi = (c_lo + 127 < A.ncols ? c_lo + 127 : A.ncols - 1);
        const int t_lo = (c_lo / A.K) >> 4, t_hi = (c_hi / A.K) >> 4;
        if (wave == 0) {
            const bool ok = wait_tiles(A.R.flags, t_lo, t_hi, A.R.flags + A.R.ntiles, lane, A.R.tmo_host);
            if (!ok && lane == 0) sq[0] = -1;
        }
    }
    __syncthreads();
    C32_TRACE_PHASE(3);   // (groups) flags seen
    int g = sq[0];
    if (FUSE == 1 && g < 0) {   // (uniform) time-out: poison the group's predictions, never hang
        for (int i = threadIdx.x; i < 128 * A.Tf2; i += blockDim.x) {
            const size_t o = (size_t)fb * 128 * A.Tf2 + i;
            if (o < (size_t)A.ncols * A.Tf2) A.pred[o] = __builtin_nanf("");
        }
        return;
    }
    if (g >= ngroups) return;  // (uniform) cannot happen with grid <= ngroups; nothing is in flight yet
    Stream st;
    st.init(A.pool, A.prog, A.prog_len, ring);

    auto col_of = [&](int gg) { int col = gg * 128 + wave * 32 + c; return col < A.ncols ? col : A.ncols - 1; };
    {   // first gathers: A0x rows of hidden tile 0, and z of this group
        const int c0 = col_of(g);
        gather_rows(A.A0x, row_off(c0 / A.K, 512, h), slot_addr);
        gather_rows(A.z, row_off(c0, 32, h), zslot_addr);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int gi = 0;
    (void)gi;
    while (true) {
        C32_STAMP(0);
        const int col = g * 128 + wave * 32 + c;
        int colc = col < A.ncols ? col : A.ncols - 1;
        int agent = colc / A.K;
        const bool live = col < A.ncols;
        // the NEXT group is requested now (one ticket of look-ahead: the last MLP prefetches its first gather); every wave reads
        // it after the many barriers of this group
        __syncthreads();  // every wave has read sq[1] of the previous hand-over before it is overwritten
        if (threadIdx.x == 0)
            sq[1] = (FUSE == 2 && A.persistent && ngroups > A.nworkers) ? A.nworkers + atomicAdd(A.counter, 1)
                    : (FUSE == 0 && A.persistent) ? atomicAdd(A.counter, 1) : ngroups;

        f32x16 acc2[8];
        f32x16 d;
        {   // ---- block 0, decoder_x: x_hat0, d = x_true - x_hat0
            agent = opaque(agent);
            f32x16 xo[1];
            const unsigned ao = row_off(agent, 512, h);
            if (B3M) {
                mlp_l12_b3<0, true>(st, slot, zslot, nullptr, A.A0x, ao, A.A0y, ao, acc2, lane);
                mlp_l3_b3<1>(st, acc2, cst + CO::b2x, cst + CO::b3x, xo, h);
            } else {
                mlp_l12<0>(st, slot, zslot, nullptr, A.A0x, ao, A.A0y, ao, acc2, lane);
                mlp_l3<1, 3>(st, acc2, cst + CO::b2x, cst + CO::b3x, xo, h);   // then decoder_y's layers 1 + 2: chunks of three
            }
            agent = opaque(agent);
            const float* xp = A.xpad + (size_t)agent * A.ldx;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                f32x4 v = splat4(0.f);
                if (8 * a + 4 * h < A.ldx) v = ld4(xp + 8 * a + 4 * h);
#pragma unroll
                for (int b = 0; b < 4; ++b) d[4 * a + b] = v[b] - xo[0][4 * a + b];
            }
        }
        STT_FENCE();
        C32_STAMP(1);
        {   // ---- block 0, decoder_y: y_hat0 parked in pred (re-read by the epilogue)
            agent = opaque(agent);
            f32x16 yo[NY];
            const unsigned ao = row_off(agent, 512, h);
            if (B3M) {
                mlp_l12_b3<0, true>(st, slot, zslot, nullptr, A.A0y, ao, A.A1y, ao, acc2, lane);
                mlp_l3_b3<NY>(st, acc2, cst + CO::b2y, cst + CO::b3y, yo, h);
            } else {
                mlp_l12<0>(st, slot, zslot, nullptr, A.A0y, ao, A.A1y, ao, acc2, lane);
                mlp_l3<NY, 1>(st, acc2, cst + CO::b2y, cst + CO::b3y, yo, h);   // then the GRU's first conv tile
            }
            if (live) {
                float* prow = A.park + (size_t)opaque(col) * A.Tf2;
#pragma unroll
                for (int o = 0; o < NY; ++o)
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const int row0 = 32 * o + 8 * a + 4 * h;
                        float* p = prow + row0;
                        if (row0 + 3 < A.Tf2 && (A.Tf2 & 3) == 0) {
                            f32x4 v = {yo[o][4 * a], yo[o][4 * a + 1], yo[o][4 * a + 2], yo[o][4 * a + 3]};
                            st4(p, v);
                        } else {
#pragma unroll
                            for (int b = 0; b < 4; ++b)
                                if (row0 + b < A.Tf2) p[b] = yo[o][4 * a + b];
                        }
                    }
            }
        }
        STT_FENCE();
        C32_STAMP(2);
        f32x16 hs[3];
        {   // ---- block 1: conv1d + relu + GRU over Tp steps, weights streamed per step
#pragma unroll
            for (int j = 0; j < 3; ++j) hs[j] = splat16(0.f);
            if (B3M) gru32_steps_b3(st, cst + CO::gb, cst + CO::cb, d, hs, A.Tp, h);
            else gru32_steps<ZS>(st, cst + CO::gb, cst + CO::cb, d, hs, A.Tp, h);
        }
        STT_FENCE();
        C32_STAMP(3);
        const int gnext = sq[1];  // written at the top of this group
        {   // ---- block 1, decoder_y + epilogue
            agent = opaque(agent);
            const int cnx = col_of(gnext < ngroups ? gnext : g);
            const unsigned ao = row_off(agent, 512, h), an = row_off(cnx / A.K, 512, h);
            if (B3M) mlp_l12_b3<3, false>(st, slot, zslot, hs, A.A1y, ao, A.A0x, an, acc2, lane);
            else mlp_l12<3>(st, slot, zslot, hs, A.A1y, ao, A.A0x, an, acc2, lane);
            // z of the NEXT group into the z slot (this group's last read of it is behind us); lands during layer 3
            gather_rows(A.z, row_off(opaque(cnx), 32, h), zslot_addr);
            f32x16 yo[NY];
            if (B3M) mlp_l3_b3<NY>(st, acc2, cst + CO::b2m, cst + CO::b3m, yo, h);
            else mlp_l3<NY, 3>(st, acc2, cst + CO::b2m, cst + CO::b3m, yo, h);   // then the program again from its start: the next group's decoder_x
            {
                agent = opaque(agent);
                const float cx = A.cur[2 * agent], cy = A.cur[2 * agent + 1];
                const float ox = A.orig[2 * agent], oy = A.orig[2 * agent + 1];
                const bool vec = (A.Tf2 & 3) == 0;
                const float* yrow = A.park + (size_t)opaque(colc) * A.Tf2;     // y_hat0 parked by this lane (dead lanes: a live column's, unused)
                float* prow = A.pred + (size_t)opaque(col) * A.Tf2;
                const float* grow = FUSE == 2 && A.m_gt ? A.m_gt + (size_t)agent * A.Tf2 : nullptr;
                float dd[NY][4][2];                                           // fused metrics: this lane's displacement norms (steps t0, t0 + 1)
#pragma unroll
                for (int o = 0; o < NY; ++o)
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const int row0 = 32 * o + 8 * a + 4 * h;
                        const bool whole = vec && row0 + 3 < A.Tf2;
                        f32x4 y0 = splat4(0.f);
                        if (whole) y0 = ld4(yrow + row0);
                        else {
#pragma unroll
                            for (int b = 0; b < 4; ++b)
                                if (row0 + b < A.Tf2) y0[b] = yrow[row0 + b];
                        }
                        f32x4 v;
                        v[0] = ((y0[0] + yo[o][4 * a + 0]) + cx) + ox;
                        v[1] = ((y0[1] + yo[o][4 * a + 1]) + cy) + oy;
                        v[2] = ((y0[2] + yo[o][4 * a + 2]) + cx) + ox;
                        v[3] = ((y0[3] + yo[o][4 * a + 3]) + cy) + oy;
                        if (live) {
                            if (whole) st4(prow + row0, v);
                            else {
#pragma unroll
                                for (int b = 0; b < 4; ++b)
                                    if (row0 + b < A.Tf2) prow[row0 + b] = v[b];
                            }
                        }
                        dd[o][a][0] = dd[o][a][1] = 0.f;
                        if (FUSE == 2 && grow) {   // (uniform)
                            if (row0 < A.Tf2) { const float2 g = *reinterpret_cast<const float2*>(grow + row0); dd[o][a][0] = bok_dist(v[0], v[1], g.x, g.y, A.m_scale); }
                            if (row0 + 2 < A.Tf2) { const float2 g = *reinterpret_cast<const float2*>(grow + row0 + 2); dd[o][a][1] = bok_dist(v[2], v[3], g.x, g.y, A.m_scale); }
                        }
                    }
                if (FUSE == 2 && grow) {   // (uniform) sum over t in order t = 0, 1, ..: lane (c, h = 0) holds steps 4a, 4a + 1 of tile row group a, lane (c, 1) steps 4a + 2, 4a + 3
                    const int Tf = A.Tf2 >> 1;
                    float acc = 0.f, fdl = -1.f;
#pragma unroll
                    for (int o = 0; o < NY; ++o)
#pragma unroll
                        for (int a = 0; a < 4; ++a) {
                            const int t0 = (32 * o + 8 * a + 4 * h) >> 1;
                            float mine = acc;
                            if (h == 0) { if (t0 < Tf) mine += dd[o][a][0]; if (t0 + 1 < Tf) mine += dd[o][a][1]; }
                            float mine1 = __shfl(mine, c, 64);
                            if (h == 1) { if (t0 < Tf) mine1 += dd[o][a][0]; if (t0 + 1 < Tf) mine1 += dd[o][a][1]; }
                            acc = __shfl(mine1, c + 32, 64);
                            if (t0 == Tf - 1) fdl = dd[o][a][0];
                            if (t0 + 1 == Tf - 1) fdl = dd[o][a][1];
                        }
                    fdl = fmaxf(fdl, __shfl_xor(fdl, 32, 64));
                    const float adev = acc / (float)Tf;
                    if (live && h == 0) {
                        atomicMin(reinterpret_cast<unsigned*>(A.m_ade) + agent, __float_as_uint(adev));
                        atomicMin(reinterpret_cast<unsigned*>(A.m_fde) + agent, __float_as_uint(fdl));
                    }
                }
            }
        }
        C32_STAMP(4);
#ifdef C32_DIAG_STAMPS
        if (threadIdx.x == 0 && A.dbg && gi < 4) {   // wave 0's chunk steps of this group: cycles barrier -> first MFMA ready, steps, an empty stamp pair
            long long* o = A.dbg + ((size_t)blockIdx.x * 4 + gi) * 16 + 10;
            o[0] = st.gap_cyc; o[1] = st.gap_n; o[2] = st.gap_cal;
        }
        st.gap_cyc = 0; st.gap_n = 0;
#endif
        ++gi;
        g = gnext;
        if (g >= ngroups) break;  // uniform: every wave read the same sq word
    }
    C32_TRACE_END(0);
}

// Stand-alone streaming GRU over columns (block 0: one column per AGENT): the same 32-column MFMA tiles and weight stream as the
// fused chain, 24 KiB of LDS and <= 256 VGPRs per wave, so its workgroups co-reside with a chain workgroup of another stream.  The
// resident-weights gru_cols kernel (144 KiB of LDS) cannot: in the pipelined form it had to wait for the running chain's tail.
struct Gru32Args {
    const float* xin; int ldx;                    // [ncols][ldx] flattened (t, c) input rows, zero padded
    const f32x4* pool; const int2* prog; int prog_len;
    const float* consts;                          // gbias[4][96] convb[32]
    float* state;                                 // [ncols][96]
    int ncols, Tp;
};
template <bool ZS>
__global__ __launch_bounds__(256, 2) void gru32_kernel(Gru32Args A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* ring = reinterpret_cast<f32x4*>(smem);
    float* cst = reinterpret_cast<float*>(ring + C32_RING);
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = threadIdx.x; i < 416; i += blockDim.x) cst[i] = A.consts[i];
    __syncthreads();
    ChainStream st;
    st.init(A.pool, A.prog, A.prog_len, ring);
    const int col = blockIdx.x * 128 + wave * 32 + c;
    const int colc = col < A.ncols ? col : A.ncols - 1;
    f32x16 d;
    {
        const float* xp = A.xin + (size_t)colc * A.ldx;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            f32x4 v = splat4(0.f);
            if (8 * a + 4 * h < A.ldx) v = ld4(xp + 8 * a + 4 * h);
#pragma unroll
            for (int b = 0; b < 4; ++b) d[4 * a + b] = v[b];
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    f32x16 hs[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) hs[j] = splat16(0.f);
    gru32_steps<ZS>(st, cst, cst + 384, d, hs, A.Tp, h);
    if (col < A.ncols) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const f32x4 v = {hs[j][4 * a], hs[j][4 * a + 1], hs[j][4 * a + 2], hs[j][4 * a + 3]};
                st4(A.state + (size_t)col * 96 + 32 * j + 8 * a + 4 * h, v);
            }
    }
}

// ---------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------
static int chain_cus() {
    static int n = 0;
    if (!n) {
        int dev = 0;
        hipDeviceProp_t p;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount;
        if (n <= 0) n = 256;
    }
    return n;
}
// STTODE_GRU_ZERO_SKIP=0: the GRUs of the chain, the throughput-form roles and gru32_kernel run gru32_steps<false> (A/B and tests only)
static int gru_zero_skip() {
    static const int v = getenv("STTODE_GRU_ZERO_SKIP") ? atoi(getenv("STTODE_GRU_ZERO_SKIP")) != 0 : 1;
    return v;
}
static int chain_lds(int NY, bool b3 = false) { return ((b3 ? 2 * C32_BUF_B3 : C32_RING) + 8 * C32_SLOT) * 16 + (1216 + 64 * NY) * 4 + 16; }

static int role_lds(int Tp) {   // agent_role's phases: embed (Tp*256 + 512 f32x4), GRU (h tiles 12 KiB + image of hidden tiles 4, 5: 48 KiB)
    const int e = (Tp * 256 + 512) * 16, g = (2 * 6 * 64 + 2 * 24 * 64 + 2 * 4 * 64) * 16;   // h tiles 12 KiB + image 48 KiB + gate hand-off 8 KiB
    return e > g ? e : g;
}

static int role32_lds() { return C32_RING * 16 + R32C::total * 4; }

template <int NY, int FUSE, bool B3M = false> static int chain_launch(ChainArgs a, int wgs_per_cu, hipStream_t s) {
    void (*kern)(ChainArgs) = gru_zero_skip() ? traj_chain_kernel<NY, FUSE, B3M, true> : traj_chain_kernel<NY, FUSE, B3M, false>;
    STT_SET_LDS_ONCE(kern, 96 * 1024);   // once per (instantiation, device): the switch is read once per process
    const int ngroups = (a.ncols + 127) / 128;
    int grid = ngroups;   // FUSE 0: one group per workgroup
    if (FUSE == 1) grid = a.R.ntiles + ngroups;   // roles ahead of their consumers, one group per workgroup
    else if (FUSE == 2) {   // another call's throughput-form roles, then this call's groups: one workgroup each, or (persistent) workers
        int workers = ngroups;
        if (a.persistent && workers > 2 * chain_cus()) workers = 2 * chain_cus();   // workers: the chip's workgroup slots
        grid = a.R32.nwg + (a.ncols > 0 ? workers : 0);
        a.nworkers = workers;
        if (workers < ngroups) a.xcd_map = 0;   // (the XCD-aware order is a permutation of one-workgroup-per-group grids)
    }
    // wgs_per_cu == 1: ask for more than half of the CU's LDS so that only ONE chain workgroup is resident per CU.  A lone workgroup
    // keeps the matrix pipe about as busy as two do (469 vs 2 x 397 us per group), and the other half of the register file plus ~76 KiB
    // of LDS stay free for kernels of OTHER streams (the separate per-agent launches of the unfused pipeline).  The fused launch needs
    // no co-residency and runs two per CU everywhere.
    int lds = chain_lds(NY, B3M);
    if (FUSE == 1 && lds < role_lds(a.Tp)) lds = role_lds(a.Tp);
    if (FUSE == 2 && a.R32.nwg > 0 && lds < role32_lds()) lds = role32_lds();
    if (wgs_per_cu == 1 && lds < 84 * 1024) lds = 84 * 1024;
    STT_REQUIRE(lds <= 96 * 1024, "sttode_traj_chain: dynamic LDS beyond the 96 KiB the kernel is registered for");
    STT_REQUIRE((long)a.ncols * 128 <= 0xffffffffL && (long)((a.ncols + a.K - 1) / a.K) * 2048 <= 0xffffffffL,
                "sttode_traj_chain: z / per-agent table rows beyond the 32-bit byte offsets of the gathers");
    if (FUSE == 1) STT_HIP(hipMemsetAsync(a.R.flags, 0, (((size_t)a.R.ntiles + 1) * 4 + 15) / 16 * 16, s));   // tile flags + time-out word
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, a);
    STT_HIP(hipGetLastError());
    return 0;
}

// DecomposeBlock front half over columns, streaming form (same function as sttode_gru_cols: model/STTODE.py:62-69).  pool / prog /
// consts: packing.gru32_stream (36 gate tiles + Tp conv tiles; 13*Tp chunk entries; gate biases [4][96] + conv bias [32]).
extern "C" int sttode_gru_cols32(const float* xin, int ldx, const float* pool, const int* prog, int prog_len, const float* consts,
                                 float* state, int ncols, int Tp, void* stream) {
    STT_REQUIRE(xin && pool && prog && consts && state, "sttode_gru_cols32: null pointer");
    STT_REQUIRE(ncols > 0 && Tp >= 1 && (ldx == 16 || ldx == 32) && 2 * Tp <= ldx, "sttode_gru_cols32: bad ncols/Tp/ldx");
    STT_REQUIRE(prog_len == 13 * Tp, "sttode_gru_cols32: chunk program must hold 13 entries per step");
    Gru32Args a;
    a.xin = xin; a.ldx = ldx; a.pool = (const f32x4*)pool; a.prog = (const int2*)prog; a.prog_len = prog_len; a.consts = consts;
    a.state = state; a.ncols = ncols; a.Tp = Tp;
    const int lds = C32_RING * 16 + 416 * 4;
    hipLaunchKernelGGL(gru_zero_skip() ? gru32_kernel<true> : gru32_kernel<false>, dim3((ncols + 127) / 128), dim3(256), lds, (hipStream_t)stream, a);
    STT_HIP(hipGetLastError());
    return 0;
}

// Stage-2 sampler's Q-net (role32.hpp qnet32) as a launch of its own: 128 agents per workgroup, 4 waves x 32 columns, the sampler's stream
// through a 24-KiB ring like gru32_kernel (<= 256 VGPRs: two workgroups per CU, beside a chain workgroup of another stream).
__global__ __launch_bounds__(256, 2) void sampler_qnet32_kernel(QNet32Args Q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* ring = reinterpret_cast<f32x4*>(smem);
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    ChainStream st;
    st.init(Q.pool, Q.prog, Q.prog_len, ring);
    const int col = blockIdx.x * 128 + wave * 32 + c;
    const bool live = col < Q.n;
    const int colc = live ? col : Q.n - 1;
    f32x16 P[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) P[kt] = ldrows(Q.pf + (size_t)colc * 128 + 32 * kt, h);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                            // chunk 0 has landed
    TileFeed<ChainStream> fd(st);
    fd.open();
    qnet32(fd, Q, P, col, colc, live, h);
    fd.close();
}

// Tiles one workgroup consumes (the program must hold exactly these): linear 8, per layer-1 tile 2 + h2/32, per sample h2/32 (x 2 with eps)
static long sampler_tiles(const SttodeSamplerPlan* p) {
    const long h1t = p->h1 / 32, h2t = p->h2 / 32;
    return 8 + h1t * (2 + h2t) + (long)p->K * h2t * (p->eps_mode ? 2 : 1);
}
const char* stt_sampler_plan_check(const SttodeSamplerPlan* p, int K) {
    if (!p || !p->pool || !p->prog || !p->biases) return "sampler plan: null pool / program / biases";
    if (p->nz != 32) return "sampler plan: nz must be 32 (one MFMA tile of rows per sample)";
    if (p->K <= 0 || (K > 0 && p->K != K)) return "sampler plan: K must be positive and equal the model's sample_k";
    if (p->h1 <= 0 || p->h1 % 32 || p->h2 <= 0 || p->h2 % 32 || p->h2 > 256) return "sampler plan: hidden widths must be multiples of 32, h2 <= 256";
    if (p->eps_mode < 0 || p->eps_mode > 2 || (p->eps_mode != 0 && !p->eps)) return "sampler plan: eps_mode 0 (mean) | 1 (shared [nz]) | 2 (per agent [n][nz]); eps required unless 0";
    if (p->prog_len <= 0 || p->prog_len > 4096) return "sampler plan: prog_len must be in [1, 4096]";
    if (3L * p->prog_len < sampler_tiles(p)) return "sampler plan: chunk program too short for the widths (<= 3 tiles per chunk)";
    return nullptr;
}
int stt_sampler_qnet(const SttodeSamplerPlan* p, const float* pf, int n, float* z, void* stream) {
    QNet32Args q;
    q.pool = (const f32x4*)p->pool; q.prog = (const int2*)p->prog; q.prog_len = p->prog_len; q.bias = p->biases;
    q.pf = pf; q.z = z; q.eps = p->eps; q.n = n; q.K = p->K; q.h1t = p->h1 / 32; q.h2t = p->h2 / 32; q.eps_mode = p->eps_mode;
    const int lds = C32_RING * 16;
    hipLaunchKernelGGL(sampler_qnet32_kernel, dim3((n + 127) / 128), dim3(256), lds, (hipStream_t)stream, q);
    STT_HIP(hipGetLastError());
    return 0;
}
extern "C" int sttode_sampler_qnet(const SttodeSamplerPlan* plan, const float* pf, int n, float* z, void* stream) {
    STT_REQUIRE(plan && pf && z, "sttode_sampler_qnet: null pointer");
    STT_REQUIRE(n > 0 && (long)n * plan->K <= 0x7fffffffL / 32, "sttode_sampler_qnet: n must be positive (and n K 32 within int range)");
    if (const char* why = stt_sampler_plan_check(plan, 0)) {
        char b[256];
        snprintf(b, sizeof(b), "sttode_sampler_qnet: %s", why);
        stt_set_error(b);
        return 1;
    }
    return stt_sampler_qnet(plan, pf, n, z, stream);
}

#if defined(C32_DIAG_STAMPS) || defined(C32_DIAG_TRACE)
static long long* g_chain_dbg = nullptr;
static int g_trace_tag = 0;
extern "C" int sttode_chain_debug_buffer(void* p) { g_chain_dbg = (long long*)p; return 0; }  // >= grid * 4 * 16 int64, zeroed
#endif

extern "C" int sttode_chain_prog_len(int Tp, int Tf) {
    const int NY = (2 * Tf + 31) / 32;
    const int l3y = (8 * NY + 2) / 3;
    return (48 + 3) + (48 + l3y) + 13 * Tp + (64 + l3y);
}

// The chain without roles; b3: the exploratory bf16-split stream (pool / prog = packing.chain_stream_b3's) instead of the fp32 one.
static int traj_chain_impl(const float* A0x, const float* A0y, const float* A1y, const float* pool, const int* prog, int prog_len,
                           const float* consts, const float* z, const float* xpad, int ldx, const float* cur, const float* orig,
                           float* pred, int* counter, int ncols, int K, int Tp, int Tf, int wgs_per_cu, bool b3, void* stream) {
    STT_REQUIRE(A0x && A0y && A1y && pool && prog && consts && z && xpad && cur && orig && pred && counter, "sttode_traj_chain: null pointer");
    STT_REQUIRE(ncols > 0 && K > 0 && Tp >= 1 && 2 * Tp <= 32 && Tf >= 1, "sttode_traj_chain: bad ncols/K/Tp/Tf");
    STT_REQUIRE(ldx == 16 || ldx == 32, "sttode_traj_chain: ldx must be 16 or 32");
    STT_REQUIRE(wgs_per_cu == 1 || wgs_per_cu == 2, "sttode_traj_chain: wgs_per_cu must be 1 or 2");
    STT_REQUIRE(2 * Tp <= ldx, "sttode_traj_chain: xpad rows shorter than 2*Tp");
    STT_REQUIRE(prog_len == sttode_chain_prog_len(Tp, Tf), "sttode_traj_chain: chunk program length does not match (Tp, Tf)");
    ChainArgs a;
    a.A0x = A0x; a.A0y = A0y; a.A1y = A1y; a.pool = (const f32x4*)pool; a.prog = (const int2*)prog; a.prog_len = prog_len;
    a.consts = consts; a.z = z; a.xpad = xpad; a.ldx = ldx; a.cur = cur; a.orig = orig; a.pred = pred; a.park = pred; a.counter = counter;
    a.ncols = ncols; a.K = K; a.Tp = Tp; a.Tf2 = 2 * Tf;
    a.dbg = nullptr; a.trace_tag = 0; a.xcd_map = 0; a.nworkers = 0; a.m_gt = nullptr; a.m_ade = a.m_fde = nullptr; a.m_scale = 1.0f;
    a.R = RoleArgs();   // unused by the unfused instantiation
    // one group per workgroup (slots free up continuously, so kernels of other streams -- the next call's per-agent stage, the next chain --
    // interleave at group granularity; measured 1.38 vs 1.87 ms per 256-scene step against workgroups pulling groups from a work queue)
    a.persistent = 0;
#if defined(C32_DIAG_STAMPS) || defined(C32_DIAG_TRACE)
    a.dbg = g_chain_dbg;
    a.trace_tag = g_trace_tag++;
#endif
    const int NY = (2 * Tf + 31) / 32;
    hipStream_t s = (hipStream_t)stream;
    if (b3) {
        switch (NY) {
            case 1: return chain_launch<1, 0, true>(a, wgs_per_cu, s);
            case 2: return chain_launch<2, 0, true>(a, wgs_per_cu, s);
            case 3: return chain_launch<3, 0, true>(a, wgs_per_cu, s);
            default: STT_REQUIRE(false, "sttode_traj_chain: future length beyond the built instantiations (2*Tf <= 96)");
        }
    }
    switch (NY) {
        case 1: return chain_launch<1, 0>(a, wgs_per_cu, s);
        case 2: return chain_launch<2, 0>(a, wgs_per_cu, s);
        case 3: return chain_launch<3, 0>(a, wgs_per_cu, s);
        default: STT_REQUIRE(false, "sttode_traj_chain: future length beyond the built instantiations (2*Tf <= 96)");
    }
    return 0;
}
// Fused per-trajectory chain of Decoder.forward (model/STTODE.py:320-347) for K samples per agent; see the file header.
extern "C" int sttode_traj_chain(const float* A0x, const float* A0y, const float* A1y, const float* pool, const int* prog, int prog_len,
                                 const float* consts, const float* z, const float* xpad, int ldx, const float* cur, const float* orig,
                                 float* pred, int* counter, int ncols, int K, int Tp, int Tf, int wgs_per_cu, void* stream) {
    return traj_chain_impl(A0x, A0y, A1y, pool, prog, prog_len, consts, z, xpad, ldx, cur, orig, pred, counter, ncols, K, Tp, Tf, wgs_per_cu, false, stream);
}
// Internal (pipeline.hip): the same on the exploratory bf16-split stream.
int stt_traj_chain_b3(const float* A0x, const float* A0y, const float* A1y, const float* pool, const int* prog, int prog_len,
                      const float* consts, const float* z, const float* xpad, int ldx, const float* cur, const float* orig,
                      float* pred, int* counter, int ncols, int K, int Tp, int Tf, int wgs_per_cu, void* stream) {
    return traj_chain_impl(A0x, A0y, A1y, pool, prog, prog_len, consts, z, xpad, ldx, cur, orig, pred, counter, ncols, K, Tp, Tf, wgs_per_cu, true, stream);
}

// Internal (csrc/pipeline.hip): the fused launch -- per-agent roles + trajectory groups in ONE grid (see RoleArgs).  W = the model's
// weight table (enum SttodeWeight), ws / off = the caller's workspace and its layout; the front-end (xpad, enc_in, cur, orig, last) has
// run on `stream` before.  attn == nullptr: attention length 1 (scene batches), the roles run the embedding too; attn != nullptr (the NBA
// branch: attention groups > 1): embed_qkv and mhgsa_attn have run on `stream` before, the roles start at the post-attention layer.
// The reference's one Euler step only.
bool stt_chain_fused_covers(int Tp) { return Tp >= 2 && 2 * Tp <= 32 && role_lds(Tp) <= 80 * 1024; }
int stt_chain_fused(const float* const* W, float* ws, const long* off, int n, int K, int Tp, int Tf, int prog_len, const float* z, float* pred,
                    float ode_time, const float* attn, int ld_attn, int wgs_per_cu, int b3, int drop_tile, unsigned* tmo_host, void* stream) {
    STT_REQUIRE(W && ws && off && z && pred, "stt_chain_fused: null pointer");
    STT_REQUIRE(n > 0 && K > 0 && stt_chain_fused_covers(Tp) && Tf >= 1, "stt_chain_fused: shape outside the fused launch");
    STT_REQUIRE(!attn || (ld_attn >= 64 && ld_attn % 4 == 0), "stt_chain_fused: bad attention leading dimension");
    STT_REQUIRE(prog_len == sttode_chain_prog_len(Tp, Tf), "stt_chain_fused: chunk program length does not match (Tp, Tf)");
    STT_REQUIRE((long)n * K <= 0x7fffffffL, "stt_chain_fused: too many trajectories");
    ChainArgs a;
    a.A0x = ws + off[STT_B_A0X]; a.A0y = ws + off[STT_B_A0Y]; a.A1y = ws + off[STT_B_A1Y];
    a.pool = (const f32x4*)W[b3 ? STT_W_CHAINB3_POOL : STT_W_CHAIN_POOL]; a.prog = (const int2*)W[b3 ? STT_W_CHAINB3_PROG : STT_W_CHAIN_PROG];
    a.prog_len = prog_len;
    a.consts = W[STT_W_CHAIN_CONSTS]; a.z = z; a.xpad = ws + off[STT_B_XPAD]; a.ldx = 2 * Tp <= 16 ? 16 : 32; a.cur = ws + off[STT_B_CUR];
    a.orig = ws + off[STT_B_ORIG]; a.pred = pred; a.park = pred; a.counter = (int*)(ws + off[STT_B_QUEUE]);
    a.ncols = n * K; a.K = K; a.Tp = Tp; a.Tf2 = 2 * Tf; a.persistent = 0; a.dbg = nullptr; a.trace_tag = 0; a.xcd_map = 0; a.nworkers = 0;
    a.m_gt = nullptr; a.m_ade = a.m_fde = nullptr; a.m_scale = 1.0f;
#if defined(C32_DIAG_STAMPS) || defined(C32_DIAG_TRACE)
    a.dbg = g_chain_dbg;
    a.trace_tag = g_trace_tag++;
#endif
    RoleArgs& r = a.R;
    role_args_fill(r, W, ws, off);
    r.attn = attn; r.ld_attn = ld_attn;
    r.past = nullptr; r.scene_ptr = nullptr; r.S = 0;   // (the scene front-end inside the role is the one-launch scene form's, scene_lat.hip)
    r.flags = (unsigned*)(ws + off[STT_B_FLAGS]); r.ntiles = (n + 15) / 16; r.ode_time = ode_time;
    r.tmo_host = tmo_host;
    a.xcd_map = 1;   // all roles sit in front of the groups: XCD-aware group order (profiles/r03/ab_xcd_map.txt)
    r.drop_tile = drop_tile;
    const int NY = (2 * Tf + 31) / 32;
    hipStream_t s = (hipStream_t)stream;
    switch (NY) {
        case 1: return b3 ? chain_launch<1, 1, true>(a, wgs_per_cu, s) : chain_launch<1, 1>(a, wgs_per_cu, s);
        case 2: return b3 ? chain_launch<2, 1, true>(a, wgs_per_cu, s) : chain_launch<2, 1>(a, wgs_per_cu, s);
        case 3: return b3 ? chain_launch<3, 1, true>(a, wgs_per_cu, s) : chain_launch<3, 1>(a, wgs_per_cu, s);
        default: STT_REQUIRE(false, "stt_chain_fused: future length beyond the built instantiations (2*Tf <= 96)");
    }
    return 0;
}

// Internal (csrc/pipeline.hip): the LAGGED launch of the pipelined path (round 4) -- ONE grid = the throughput-form per-agent roles of one
// call (role32.hpp: 128 agents per workgroup; rW / ws_r / off_r / n_r; skipped when ws_r == nullptr) followed by the trajectory groups of
// ANOTHER, earlier call whose roles ran in an earlier launch of the same stream (ws_g / off_g / n_g / z / pred; skipped when ws_g ==
// nullptr).  Nothing in the grid depends on anything else in it.  attn != nullptr (NBA: attention groups > 1): embed_qkv and mhgsa_attn of
// the roles' call have run on `stream` before, the roles read g and the attention output from ws_r.  The reference's one Euler step only.
bool stt_chain_lagged_covers(int Tp) { return Tp >= 2 && 2 * Tp <= 32; }
int stt_chain_lagged(const float* const* W, const LagRoles& lr, const LagGroups& lg, int K, int Tp, int Tf, int prog_len, int b3, void* stream) {
    float* ws_r = lr.ws; const long* off_r = lr.off; const int n_r = lr.n; const float* attn = lr.attn; const int ld_attn = lr.ld_attn;
    const float ode_time = lr.ode_time; float* zgen = lr.zgen; const unsigned long long zkey = lr.zkey; const float* past = lr.past;
    const int* scene_ptr = lr.scene_ptr; const int S = lr.S; float* r_ade = lr.ade; float* r_fde = lr.fde;
    float* ws_g = lg.ws; const long* off_g = lg.off; const int n_g = lg.n; const float* z = lg.z; float* pred = lg.pred;
    const float* g_gt = lg.gt; float* g_ade = lg.ade; float* g_fde = lg.fde; const float g_scale = lg.scale; const int lag_workers_ok = lg.workers;
    STT_REQUIRE(W && (ws_r || ws_g), "stt_chain_lagged: nothing to launch");
    STT_REQUIRE(K > 0 && stt_chain_lagged_covers(Tp) && Tf >= 1, "stt_chain_lagged: shape outside the lagged launch");
    ChainArgs a;
    a.R = RoleArgs();
    a.R32 = Role32Args();
    a.dbg = nullptr; a.trace_tag = 0; a.xcd_map = 0; a.persistent = 0; a.counter = nullptr; a.nworkers = 0;
    a.K = K; a.Tp = Tp; a.Tf2 = 2 * Tf; a.ldx = 2 * Tp <= 16 ? 16 : 32; a.ncols = 0;
    a.pool = (const f32x4*)W[b3 ? STT_W_CHAINB3_POOL : STT_W_CHAIN_POOL]; a.prog = (const int2*)W[b3 ? STT_W_CHAINB3_PROG : STT_W_CHAIN_PROG];
    a.prog_len = prog_len; a.consts = W[STT_W_CHAIN_CONSTS];
    a.A0x = a.A0y = a.A1y = nullptr; a.z = nullptr; a.xpad = nullptr; a.cur = a.orig = nullptr; a.pred = nullptr; a.park = nullptr;
    a.m_gt = nullptr; a.m_ade = a.m_fde = nullptr; a.m_scale = 1.0f;
    if (ws_g && g_gt) {
        STT_REQUIRE(g_ade && g_fde, "stt_chain_lagged: fused metrics need ade and fde");
        a.m_gt = g_gt; a.m_ade = g_ade; a.m_fde = g_fde; a.m_scale = g_scale;
    }
    if (ws_g) {
        STT_REQUIRE(off_g && z && pred && n_g > 0 && (long)n_g * K <= 0x7fffffffL, "stt_chain_lagged: bad group arguments");
        STT_REQUIRE(prog_len == sttode_chain_prog_len(Tp, Tf), "stt_chain_lagged: chunk program length does not match (Tp, Tf)");
        a.A0x = ws_g + off_g[STT_B_A0X]; a.A0y = ws_g + off_g[STT_B_A0Y]; a.A1y = ws_g + off_g[STT_B_A1Y];
        a.z = z; a.xpad = ws_g + off_g[STT_B_XPAD]; a.cur = ws_g + off_g[STT_B_CUR]; a.orig = ws_g + off_g[STT_B_ORIG]; a.pred = pred;
        a.park = ws_g + off_g[STT_B_YBUF];   // (m x 16 NOY floats >= m x 2 Tf): the kernel never reads `pred`, which may be pinned host memory
        a.ncols = n_g * K;
        // Workers: the launch holds at most the chip's 2-per-CU workgroup slots, and its workgroups pull groups from the call's work queue.
        // One workgroup per group deals the groups to the 8 XCDs statically (block % 8), the next launch on another queue starts only when
        // this grid is fully dispatched, and the XCDs do not run at one speed: the block trace shows six XCDs idle for 250-700 us at the end
        // of every launch while the slowest still has blocks to place (profiles/r04/trace_lagged_static.txt)
        // (calls with launches in front of the roles -- the NBA branch's front-end, embedding and attention -- keep one workgroup per group:
        // workers hold every slot until their queue is empty and those kernels would wait for the launch's end; measured -8 % there)
        a.persistent = lag_workers_ok ? 1 : 0;
        a.counter = (int*)(ws_g + off_g[STT_B_QUEUE]);       // zeroed by the roles of this call (an earlier launch of this stream)
        a.xcd_map = 1;
    }
    if (ws_r) {
        STT_REQUIRE(off_r && n_r > 0, "stt_chain_lagged: bad role arguments");
        STT_REQUIRE(!attn || (ld_attn >= 64 && ld_attn % 4 == 0), "stt_chain_lagged: bad attention leading dimension");
        Role32Args& r = a.R32;
        r.pool = (const f32x4*)W[STT_W_ROLE32_POOL];
        r.prog = (const int2*)W[attn ? STT_W_ROLE32_PROG_NBA : STT_W_ROLE32_PROG_SCENES];
        r.consts = W[attn ? STT_W_ROLE32_CONSTS_NBA : STT_W_ROLE32_CONSTS_SCENES];
        r.kte = (4 * Tp + 31) / 32;
        const int e = attn ? 8 : 2 * r.kte + 8;   // == packing.role_prog_len
        r.prog_len = attn ? 13 * Tp + (e + 2) / 3 + (128 + 288 + 2) / 3 : 13 * Tp + (e + 128 + 288 + 2) / 3;
        r.enc_in = ws_r + off_r[STT_B_ENC_IN]; r.last = (const int*)(ws_r + off_r[STT_B_LAST]);
        r.g_in = ws_r + off_r[STT_B_G]; r.attn = attn; r.ld_attn = ld_attn;
        r.xpad = ws_r + off_r[STT_B_XPAD]; r.ldx = a.ldx;
        r.pf = ws_r + off_r[STT_B_PF]; r.state0 = ws_r + off_r[STT_B_STATE0];
        r.A0x = ws_r + off_r[STT_B_A0X]; r.A0y = ws_r + off_r[STT_B_A0Y]; r.A1y = ws_r + off_r[STT_B_A1Y];
        r.n = n_r; r.Tp = Tp; r.nwg = (n_r + 127) / 128; r.ode_time = ode_time;
        r.prio = 3;   // role waves outlast the groups of a small launch: SDD-256 / NBA-128 +1..2 %, 512 scenes the same (profiles/r04/role_prio_ab.txt)
        r.counter = (int*)(ws_r + off_r[STT_B_QUEUE]);
        r.zgen = zgen; r.zkey0 = (unsigned)zkey; r.zkey1 = (unsigned)(zkey >> 32); r.K = K;
        STT_REQUIRE(!past || (scene_ptr && S > 0 && !attn), "stt_chain_lagged: the in-role front-end needs scene_ptr, S > 0 and attention length 1");
        r.past = past; r.scene_ptr = scene_ptr; r.S = S;
        r.scene_orig = ws_r + off_r[STT_B_SCENE_ORIG]; r.agent_scene = (int*)(ws_r + off_r[STT_B_AGENT_SCENE]);
        r.enc_in_w = ws_r + off_r[STT_B_ENC_IN]; r.xpad_w = ws_r + off_r[STT_B_XPAD]; r.cur_w = ws_r + off_r[STT_B_CUR];
        r.orig_w = ws_r + off_r[STT_B_ORIG]; r.last_w = (int*)(ws_r + off_r[STT_B_LAST]);
        r.m_ade = r_ade; r.m_fde = r_fde;
    }
#if defined(C32_DIAG_STAMPS) || defined(C32_DIAG_TRACE)
    a.dbg = g_chain_dbg;
    a.trace_tag = g_trace_tag++;
#endif
    const int NY = (2 * Tf + 31) / 32;
    hipStream_t s = (hipStream_t)stream;
    switch (NY) {
        case 1: return b3 ? chain_launch<1, 2, true>(a, 2, s) : chain_launch<1, 2>(a, 2, s);
        case 2: return b3 ? chain_launch<2, 2, true>(a, 2, s) : chain_launch<2, 2>(a, 2, s);
        case 3: return b3 ? chain_launch<3, 2, true>(a, 2, s) : chain_launch<3, 2>(a, 2, s);
        default: STT_REQUIRE(false, "stt_chain_lagged: future length beyond the built instantiations (2*Tf <= 96)");
    }
    return 0;
}
