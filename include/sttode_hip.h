/* sttode_hip.h -- C ABI of libsttode_hip.so (MI355X / gfx950), the drop-in boundary of the STTODE
 * forward trajectory-forecasting hot path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 (or int32 where noted) owned by the caller;
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream), nothing
 *     synchronises, nothing allocates: all workspaces are caller-provided (graph-capturable; a workspace of the native pipeline is
 *     initialised ONCE with sttode_workspace_init before its first use);
 *   - threads: the per-kernel entry points are re-entrant (no state); the asynchronous entry points of ONE SttodeModel (sttode_inference_*_async,
 *     sttode_wait*, sttode_async_*, sttode_set_lagged) are serialised by a mutex inside the model and take everything a call needs as
 *     arguments (no arm-then-call state) -- but the ORDER of calls decides which slot's groups a launch carries and which stream
 *     sttode_async_next_stream names, so a model's pipelined calls belong to one host thread at a time; serial calls on different
 *     workspaces may come from different threads;
 *   - return 0 on success, non-zero on failure; sttode_last_error() gives the calling thread's message;
 *   - "PK16" = weights pre-packed in MFMA fragment order by sttode_amd/packing.py (csrc/chain.hpp);
 *   - "columns" are agents (n) or trajectories (m = n*K, row = agent*K + k, model/STTODE.py:322-328).
 *
 * Each entry point names the reference interface it replaces (file:line in joyecnu/STTODE).
 */
#ifndef STTODE_HIP_H
#define STTODE_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header: the library returns it from sttode_abi_version(); a binding compares before its first call (round 1-2: 1). */
#define STTODE_ABI_VERSION 15
int sttode_abi_version(void);
const char* sttode_last_error(void);

/* Train-mode augmentation of set_data (model/STTODE.py:417-426, rotation_2d_torch :6-14): past [n,Tp,2] and fut [n,Tf,2] (optional) rotated in
 * place about the mean of the agents' last observed positions by the angle with cosine c and sine s.  One scene per call. */
int sttode_rotate_scene(float* past, float* fut, int n, int Tp, int Tf, float c, float s, void* stream);

/* STTODENet.set_data (model/STTODE.py:397-461), batched over S independent scenes (CSR scene_ptr ==
 * seq_start_end, utils/dataloader.py:177-181): scene_orig = mean_n(last obs) (:417), normalised past (:429),
 * first-difference velocities with the first duplicated (:432-433 / inference :588-589), cur_location (:461),
 * last-agent flag for add_category (:206).  past [n,Tp,2] world coords; outputs: scene_orig [S,2],
 * agent_scene [n] int32, xpad [n,16*TPX] (flattened (t,c), zero padded), enc_in [n,Tp,4], cur [n,2],
 * orig [n,2] (scene_orig per agent), last_flag [n] int32.  vel_from_norm: 1 = inference() semantics. */
int sttode_frontend_scenes(const float* past, const int* scene_ptr, int n, int S, int Tp, int TPX, int vel_from_norm,
                           float* scene_orig, int* agent_scene, float* xpad, float* enc_in, float* cur, float* orig,
                           int* last_flag, void* stream);

/* STTODENet.set_data_nba / inference() NBA branch (model/STTODE.py:463-486,578-583): past [B*N,Tp,2], no
 * normalisation, orig = 0, last_flag = (slot == N-1). */
int sttode_frontend_nba(const float* past, int n, int N, int Tp, int TPX, float* xpad, float* enc_in, float* cur, float* orig,
                        int* last_flag, void* stream);

/* inputs_for_posterior (model/STTODE.py:430,434,457 ; 477,481): future [n,Tf,2], past_last [n,2] world. */
int sttode_frontend_future(const float* future, const float* past_last, int n, int Tf, int mode, int nba_N,
                           const float* scene_orig, const int* agent_scene, const int* scene_ptr, float* enc_in, void* stream);

/* PastEncoder.forward up to the attention in-projection (model/STTODE.py:214-223; PositionalAgentEncoding
 * :167-176; add_category :199-210; Hyp_mhsa packed in-proj hyptransformerlib.py:113-115).
 * enc_in [n,Tlen,4] -> g [n,64] (ftraj_input), qkv [n,192] (raw q|k|v, q NOT yet scaled). */
int sttode_embed_qkv(const float* fc1P, const float* fc1b, const float* posP, const float* peb, const float* fc2P,
                     const float* fc2b, const float* fc3P, const float* fc3b, const float* fc3last, const float* inP,
                     const float* inb, const float* enc_in, const int* last_flag, float* g, float* qkv, int n, int Tlen,
                     void* stream);

/* Multi-head geodesic attention core, 8 heads x 8 dims (hyptransformerlib.py:191,214-218,251-300;
 * Oblique.proj/dist core/manifolds/oblique.py:15-16,36-43):
 *   out_i = sum_j softmax_j( -acos(clamp(<r_i/|r_i|, c_j/|c_j|>, -1+1e-4, 1-1e-4)) ) v_j
 * element (seq s, batch b, feature f) at base + s*seq_stride + b*batch_stride + f (strides in floats).
 * Self-attention L == S (the reference's live path): R = k, C = q (cscale = hd^-0.5), i.e. the untransposed-score
 * quirk (:261-265).  L != S: R = q (rscale = hd^-0.5), C = k.  rowsum [Nb,8,rows] and wout [Nb,rows,cols]
 * (head-averaged weights, :306-309) are optional. */
int sttode_mhgsa_attn(const float* R, const float* C, const float* V, float* out, float* rowsum, float* wout, int rows,
                      int cols, int Nb, long rs_seq, long rs_b, long cs_seq, long cs_b, long vs_seq, long vs_b, long os_seq,
                      long os_b, float rscale, float cscale, void* stream);
/* The same core over `groups` independent problems of one shape in ONE launch: group g reads R + g gs_r, C + g gs_c, V + g gs_v and writes
 * out + g gs_o (strides in floats).  The NBA branch attends over the batch dimension of ONE forward call (hyptransformerlib.py:261-265); a
 * test set is many such batches (test.py:520-524), and one launch over all of them fills the chip.  head_dim = hidden_dim / 8: 8 for the
 * reference default, 4 / 16 for --hidden_dim 32 / 128 (train.py:38; features of head h at offset h head_dim). */
int sttode_mhgsa_attn_groups(const float* R, const float* C, const float* V, float* out, int groups, long gs_r, long gs_c, long gs_v, long gs_o,
                             int rows, int cols, int Nb, long rs_seq, long rs_b, long cs_seq, long cs_b, long vs_seq, long vs_b, long os_seq,
                             long os_b, float rscale, float cscale, int head_dim, void* stream);
/* Attention core with a running maximum (csrc/attention.hip; added within ABI version 14): operands and strides as sttode_mhgsa_attn,
 * 8 heads x 8 dims.  mode 0: the geodesic scores above (hyptransformerlib.py:251-300); mode 1: dot-product scores
 * s_ij = <rscale R_i, cscale C_j>, no normalisation, no clamp (transformerlib.py:251-282: R = q, rscale = hd^-0.5).  mask: NULL, or an fp32
 * [rows, cols] additive mask with row stride ld_mask >= cols floats, shared by every slot and head: mask[i * ld_mask + j] is added to score
 * (row i, column j) before the softmax (hyptransformerlib.py:290-292, transformerlib.py:276-279); -inf and +inf entries are allowed, NaN
 * entries are unspecified.  A row that is -inf over all columns yields a NaN output row and NaN weights (torch's softmax does); other
 * rows of the call are unaffected.  wmax / wsum [Nb,8,rows] (both or neither): the softmax's per-(slot, head, row) maximum and sum of
 * exp(s - max); wout [Nb,rows,cols] (head-averaged weights) needs them.  Deterministic bit for bit; no host synchronisation and no
 * allocation (safe under stream capture). */
int sttode_attn_core(const float* R, const float* C, const float* V, const float* mask, long ld_mask, float* out, float* wmax, float* wsum,
                     float* wout, int rows, int cols, int Nb, long rs_seq, long rs_b, long cs_seq, long cs_b, long vs_seq, long vs_b,
                     long os_seq, long os_b, float rscale, float cscale, int mode, void* stream);
/* Backward of sttode_attn_core: dO laid out like `out` (strides os_*) -> dR, dC, dV in the layouts of R, C, V (overwritten, not
 * accumulated).  Mode 0: through the clamp (torch.clamp, bounds inclusive), both normalisations and both scales; mode 1: through both
 * scales.  Positions masked with -inf have probability 0 and contribute nothing; the mask gets no gradient.  One workgroup per
 * (slot, head), deterministic; rows (2 head_dim + 3) + cols 2 head_dim floats of LDS must fit 64 KiB (rows = cols <= 468). */
int sttode_attn_core_bwd(const float* R, const float* C, const float* V, const float* mask, long ld_mask, const float* dO, float* dR,
                         float* dC, float* dV, int rows, int cols, int Nb, long rs_seq, long rs_b, long cs_seq, long cs_b, long vs_seq,
                         long vs_b, long os_seq, long os_b, float rscale, float cscale, int mode, void* stream);

/* out_proj (hyptransformerlib.py:305) -> Hypattention gate tanh(info)*sigmoid(gate) (hypertransformer.py:81-83)
 * -> TransformerEncoderLayer post-LN + FFN (hypertransformer.py:148-152) -> ODEG_Encoder: one explicit Euler step of
 * size ode_time and relu (ode_demo.py:186-190,223-231) -> pf [n,128] = cat(g, ode) (model/STTODE.py:233-235). */
int sttode_post_attn(const float* outP, const float* outb, const float* infoP, const float* infob, const float* gateP,
                     const float* gateb, const float* ln1w, const float* ln1b, const float* l1P, const float* l1b,
                     const float* l2P, const float* l2b, const float* ln2w, const float* ln2b, const float* g, const float* attn,
                     int ld_attn, float* pf, int n, float ode_time, void* stream);

/* The same layer with the integrator as a kernel parameter (the north star names RK4 / multi-step updates; the reference itself only ever
 * runs ONE Euler step, ode_demo.py:186-190, so anything else is checked against the CPU oracle only: parity unpinned).
 * method 0 Euler | 1 torchdiffeq fixed-grid "rk4" (3/8 rule) | 2 classical RK4; `steps` uniform steps over [0, ode_time].  Attention
 * length 1 only (ETH/UCY/SDD path: the attention output of a stage's state is W_v y + b_v, taken from the packed in-projection
 * inP/inb and evaluated inside the kernel); (method 0, steps 1) equals sttode_post_attn. */
int sttode_post_attn_ode(const float* outP, const float* outb, const float* infoP, const float* infob, const float* gateP,
                         const float* gateb, const float* ln1w, const float* ln1b, const float* l1P, const float* l1b,
                         const float* l2P, const float* l2b, const float* ln2w, const float* ln2b, const float* inP, const float* inb,
                         const float* g, float* pf, int n, float ode_time, int method, int steps, void* stream);

/* Right-hand side of the encoder's tensor ODE at ONE state y [n,64] for any attention length: k = LN2(h + FFN(h)), h = LN1(y + gate(out_proj(a)))
 * with `a` [n, ld_attn] the attention output of state y (TransformerEncoder_ode.forward, ode_demo.py:25-72 = TransformerEncoderLayer.forward,
 * hypertransformer.py:134-153).  The native pipeline integrates with it when a non-default integrator meets an attention group > 1:
 * per stage in-projection of y (sttode_linear_cols) -> sttode_mhgsa_attn over the group -> this -> axpy combinations. */
int sttode_post_attn_rhs(const float* outP, const float* outb, const float* infoP, const float* infob, const float* gateP,
                         const float* gateb, const float* ln1w, const float* ln1b, const float* l1P, const float* l1b,
                         const float* l2P, const float* l2b, const float* ln2w, const float* ln2b, const float* y,
                         const float* attn, int ld_attn, float* kout, int n, void* stream);
/* past_feature [n,128] = cat(ftraj_input g, relu(integrated ODE state y)) (ode_demo.py:231, model/STTODE.py:233-235) */
int sttode_ode_state_to_pf(const float* g, const float* y, float* pf, int n, void* stream);

/* DecomposeBlock front half (model/STTODE.py:62-69): conv1d(2->32,k3,pad1)+relu, GRU(32->96) final state.
 * xin [ncols,16*TPX] = flattened (x_true - x_hat) -> state [ncols,96]. */
int sttode_gru_cols(const float* xin, const float* convP, const float* convB, const float* wihP, const float* whhP,
                    const float* gbias, float* state, int ncols, int Tp, int TPX, void* stream);

/* Process-wide crossover between the latency forms of sttode_gru_cols / sttode_mlp_block0 / sttode_mlp_block1 / sttode_embed_qkv (one
 * 16-column tile per WORKGROUP, its waves splitting the rows: a single scene of test.py:171-188) and their throughput forms (a tile per
 * wave): the latency form serves calls of at most this many 16-column tiles.  Negative = leave unchanged; defaults 512 / 1024 / 1024.
 * Both forms sum in the same order: results are bitwise independent of the setting. */
int sttode_set_latency_tiles(int gru_tiles, int mlp_tiles, int enc_tiles);

/* Generic per-column linear out[col, 0:N] = act(W [X1 | X2] + b) (nn.Linear; used for the per-agent part of
 * decoder_x/decoder_y layer 0, model/utils.py:86-95, and for the stage-2 Q-net, sampler.py:39,48-52 / utils/mlp.py:26-29).
 * K1, K2, N multiples of 16.  act: 0 none, 1 relu, 2 tanh. */
int sttode_linear_cols(const float* X1, int ld1, int K1, const float* X2, int ld2, int K2, const float* WP, const float* bias,
                       float* out, int ldo, int ncols, int N, int act, void* stream);

/* The three per-agent layer-0 pre-activations of decoder_x/decoder_y (block 0) and decoder_y (block 1) in one launch:
 * A0x, A0y = W[:, pf|state] [pf | state0] + b ; A1y = W[:, pf] pf + b   (model/STTODE.py:71,74-75 split). */
int sttode_agent_preact(const float* pf, const float* state0, const float* WAx, const float* b1x, const float* WAy,
                        const float* b1y, const float* WA1, const float* b11, float* A0x, float* A0y, float* A1y, int n,
                        void* stream);

/* DecomposeBlock 0 back half for all K samples (model/STTODE.py:71-75, Decoder.forward :336-339):
 * decoder_x and decoder_y MLPs; writes dbuf = x_true - x_hat0 [m,16*TPX] and ybuf = y_hat0 [m,16*NOY].
 * A0x/A0y [n,512]: per-agent part of layer 0 (sttode_linear_cols); stream: packed weight-chunk stream of both MLPs
 * (packing.mlp_stream: fragment-ordered 18 KiB chunks, layer-2/3 biases inside), total_chunks = (32 + TPX) + (32 + NOY). */
int sttode_mlp_block0(const float* A0x, const float* A0y, const float* stream, int total_chunks,
                      const float* z, const float* xpad, float* dbuf, float* ybuf, int ncols, int K, int TPX, int NOY,
                      void* stream_);

/* DecomposeBlock 1 back half + Decoder epilogue (model/STTODE.py:338,343-346) + "+ scene_orig" (:621-622):
 * pred [m,Tf,2] = ((y_hat0 + y_hat1) + cur_location) + scene_orig.  total_chunks = 32 + NOY (24 KiB chunks). */
int sttode_mlp_block1(const float* A1y, const float* stream, int total_chunks, const float* z,
                      const float* state1, const float* ybuf, const float* cur, const float* orig, float* pred, int ncols,
                      int K, int Tf, int NOY, void* stream_);

/* One decoder MLP of a non-first DecomposeBlock with B = [z | state] per column (model/STTODE.py:71-75): raw output tiles
 * out [ncols,16*NO].  Used by the training-forward path for the last block's decoder_x (recover_traj, :339-341). */
int sttode_mlp_cols(const float* A0, const float* stream, int total_chunks, const float* z,
                    const float* state, float* out, int ncols, int K, int NO, void* stream_);

/* Fused per-trajectory chain of Decoder.forward for all K samples (model/STTODE.py:320-347 with DecomposeBlock.forward :51-77
 * twice and the "+ scene_orig" of :621-622): block-0 decoder_x -> d = x_true - x_hat0 -> block-0 decoder_y -> block-1 conv + GRU
 * -> block-1 decoder_y -> pred [m,Tf,2] = ((y_hat0 + y_hat1) + cur) + orig, ONE persistent kernel, intermediates in registers
 * (replaces sttode_mlp_block0 + sttode_gru_cols + sttode_mlp_block1 on the inference path; csrc/chain32.hip).
 * A0x/A0y/A1y [n,512] as above; pool/prog/consts: packing.chain_stream (PK32 tile pool, per-group chunk program of
 * sttode_chain_prog_len(Tp,Tf) int32 pairs, bias block); xpad [n,ldx] (ldx = 16 or 32); counter: one int32 of scratch
 * (work queue, zeroed by the call on `stream`); wgs_per_cu: resident workgroups per CU, 2 for a stand-alone call, 1 when kernels of
 * other streams should run beside it (the pipelined forms use 1). */
int sttode_traj_chain(const float* A0x, const float* A0y, const float* A1y, const float* pool, const int* prog, int prog_len,
                      const float* consts, const float* z, const float* xpad, int ldx, const float* cur, const float* orig,
                      float* pred, int* counter, int ncols, int K, int Tp, int Tf, int wgs_per_cu, void* stream);
int sttode_chain_prog_len(int Tp, int Tf);
/* sttode_gru_cols in streaming form (same function: DecomposeBlock front half, model/STTODE.py:62-69): 32-column MFMA tiles, every
 * weight tile streamed per step, 24 KiB of LDS -- its workgroups co-reside with a running sttode_traj_chain of another stream, which
 * the resident-weights kernel (144 KiB of LDS) cannot.  pool / prog / consts: packing.gru32_stream; prog_len = 13 * Tp; ldx = 16 | 32. */
int sttode_gru_cols32(const float* xin, int ldx, const float* pool, const int* prog, int prog_len, const float* consts, float* state,
                      int ncols, int Tp, void* stream);

/* compute_ADE / compute_FDE per agent (utils/metrics.py:7-26): pred [n,K,Tf,2], gt [n,Tf,2] -> ade [n], fde [n]; any K >= 1.
 * Non-finite samples: a sample whose mean (final) displacement is NaN is skipped by the minimum (fminf); an agent whose samples are all
 * NaN gets +inf, at any K. */
int sttode_best_of_k(const float* pred, const float* gt, int n, int K, int Tf, float scale, float* ade, float* fde, void* stream);
/* The NBA evaluation's per-horizon metric (test.py:530-551): pred [n,K,Tf,2], gt [n,Tf,2] -> out [n,Tf,2]: for agent a and horizon h (frame
 * h - 1) out[a][h-1] = (min_k mean_{t < h} |scale (pred - gt)|, min_k |scale (pred_h - gt_h)|); the caller averages over agents and weighs by
 * the batch size like the reference.  K <= 64, K Tf <= 2048. */
int sttode_horizon_metrics(const float* pred, const float* gt, int n, int K, int Tf, float scale, float* out, void* stream);
/* Best-of-K selection per agent and per segment: compute_ADE / compute_FDE (utils/metrics.py:7-26), get_best_idx (:29-36) and
 * count_miss_samples (:39-48), the per-agent loop of test.py:193-205 (its ade per scene: :201-205).  pred [n,K,Tf,2], gt [n,Tf,2], K <= 64
 * (refused above that, nothing written).  Per agent: ade [n], fde [n] (the bits of sttode_best_of_k for every agent with at least one
 * finite sample); best_ade_idx / best_fde_idx [n] = argmin
 * over k of the mean / final displacement, the lowest k on exact ties (np.argmin); miss [n] = fde > miss_threshold (1 / 0, strictly);
 * best [n,Tf,2] = pred[a, best_ade_idx[a]] (copied, unscaled).  Per segment s of the CSR seg_ptr [S+1] (scene_ptr; B segments of N for NBA):
 * seg_ade / seg_fde [S] = mean over agents seg_ptr[s] .. seg_ptr[s+1]-1, seg_miss [S] = their miss count, summed in a fixed order (no
 * atomics: the same bits on every run); segment bounds are clamped to [0, n] with the end no lower than the start, and an empty segment
 * gets NaN means and a zero count.  Every output but ade / fde may be NULL; seg_ptr may be NULL (S = 0) when no segment output is asked.
 * Non-finite samples: a NaN sample is skipped, as in sttode_best_of_k, and never chosen.  An agent whose samples are all NaN gets index 0
 * for both indices, best = its sample 0 (the gather stays inside the agent), and ade / fde = +inf at K < 64 (the idle lanes hold +inf; a
 * miss) but NaN at K = 64 (every lane holds a NaN; NaN > miss_threshold is false: not a miss) -- there, and only there, its ade / fde are
 * not sttode_best_of_k's +inf. */
int sttode_best_of_k_select(const float* pred, const float* gt, int n, int K, int Tf, float scale, float miss_threshold, const int* seg_ptr,
                            int S, float* ade, float* fde, int* best_ade_idx, int* best_fde_idx, unsigned char* miss, float* best,
                            float* seg_ade, float* seg_fde, int* seg_miss, void* stream);
/* Scene-level metrics of K sampled futures.  The reference computes none of them, so there is no line of it to cite.
 * pred [n,K,Tf,2], gt [n,Tf,2] (float32, device), coordinates multiplied by `scale`; a segment s of the CSR seg_ptr [S+1] (a scene, or one
 * NBA game of N players) is the agents seg_ptr[s] .. seg_ptr[s+1]-1.  Both entry points refuse a K they do not take before anything is
 * written; there are no atomics and every sum has a fixed order: the same bits on every run.
 * sttode_joint_select (1 <= K <= 64):
 *   ADE(a, k) / FDE(a, k): per-(agent, sample) mean / final displacement, the bits bok_select_kernel computes for lane k (a one-agent
 *   segment reproduces sttode_best_of_k_select's ade / fde / best_ade_idx / best_fde_idx bitwise).
 *   seg_jade[s] = min_k (sum over the segment's agents of ADE(a, k), in double, / agent count) as float32; seg_jade_idx[s] = its k, the
 *   lowest on exact ties of the double values (np.argmin); seg_jfde / seg_jfde_idx the same of FDE.  An empty segment gets NaN, index 0.
 *   radius > 0: agent a collides in sample k if some other agent b of its segment has dx^2 + dy^2 < radius^2 (strictly; dx, dy float32
 *   differences of the scaled coordinates) at some frame; seg_col[s] = sum over k of the colliding agents of sample k, seg_gt_col[s] =
 *   the colliding agents of gt.  A one-agent segment has none.  radius <= 0: no collision pass; seg_col / seg_gt_col may be NULL.
 * sttode_kde_nll (2 <= K <= 64), Trajectron++'s compute_kde_nll (scipy.stats.gaussian_kde per agent and frame), all in float64 with
 *   x = (double)(x * scale): per frame C = the unbiased (/ (K-1)) 2 x 2 covariance of the K samples, Sigma = f^2 C with Scott's factor
 *   f = K^(-1/6), logpdf = logsumexp_k(-(g - x_k)^T Sigma^-1 (g - x_k) / 2) - log K - log det(2 pi Sigma) / 2 clipped below at -20;
 *   nll [n] = -mean over frames.  NaN if C is not positive definite at some frame (C00 <= 0 or det C <= 0: where gaussian_kde raises). */
int sttode_joint_select(const float* pred, const float* gt, int n, int K, int Tf, float scale, const int* seg_ptr, int S, float radius,
                        float* seg_jade, float* seg_jfde, int* seg_jade_idx, int* seg_jfde_idx, int* seg_col, int* seg_gt_col, void* stream);
int sttode_kde_nll(const float* pred, const float* gt, int n, int K, int Tf, float scale, double* nll, void* stream);
/* Spread of the K sampled futures of every agent among themselves; the reference has only the DLow term, as a training loss
 * (samplerloss.py:12-20).  pred [n,K,Tf,2] float32, gt [n,Tf,2] float32 or NULL; n >= 1, 2 <= K <= 64, Tf >= 1, div_scale > 0 and finite.
 * Coordinates are x = (double)(x * scale), the product in float32 as sttode_kde_nll; everything after that is float64.  For the pairs
 * i < j of an agent's samples, in F.pdist order, frames summed in frame order and pairs in pair order:
 *   d_traj(i,j) = sqrt(sum_t |x_i,t - x_j,t|^2),  d_ade(i,j) = (1/Tf) sum_t |x_i,t - x_j,t|,  d_fde(i,j) = |x_i,Tf-1 - x_j,Tf-1|.
 * Per agent, float64 [n] (required):
 *   apd  = mean over the K(K-1)/2 pairs of d_traj (DLow's APD: pdist of the flattened trajectories);  fpd = mean of d_fde;
 *   pade = mean of d_ade;  dlow = mean of exp(-d_traj^2 / div_scale): the per-agent term of diversity_loss, dlow.sum() / n its
 *   loss_unweighted.
 * With gt (each may be NULL; all must be NULL when gt is NULL):
 *   es_ade [n] = (1/K) sum_k D_ade(x_k, y) - ((K-1)/(2K)) pade,  es_fde [n] = (1/K) sum_k D_fde(x_k, y) - ((K-1)/(2K)) fpd: the energy
 *   score E|X - y| - E|X - X'|/2 of the ensemble with the 1/K^2 double sum, D_ade / D_fde the same float64 distances to the ground truth.
 *   ade_at_k / fde_at_k [n,K] float32: column k-1 = the minimum over the first k samples of ADE(a, .) / FDE(a, .), the float32 values of
 *   bok_select_kernel (NaN samples skipped): column K-1 is sttode_best_of_k_select's ade / fde bit for bit, and column k-1 what it gives
 *   for the first k samples (+inf if all of them are NaN and k < 64, as there).
 * Refused before any launch or write, naming the entry.  No atomics, every sum in a fixed order: the same bits on every run. */
int sttode_sample_spread(const float* pred, const float* gt, int n, int K, int Tf, float scale, double div_scale, double* apd, double* fpd,
                         double* pade, double* dlow, double* es_ade, double* es_fde, float* ade_at_k, float* fde_at_k, void* stream);
/* A weighted sample set against the ground truth (added within ABI version 15): K representatives per agent with raw weights
 * (sttode_reduce_samples' counts, counts / M, or mode probabilities).  The reference computes none of this; kde_nll stands for
 * Trajectron++'s compute_kde_nll over scipy.stats.gaussian_kde(dataset, weights=w), the rest for the probability-ranked minADE_k / minFDE_k,
 * brier-minFDE and energy score of Argoverse / Waymo style tables.
 * pred [n,K,Tf,2], weights [n,K], gt [n,Tf,2] float32; n >= 1, 1 <= K <= 64, Tf >= 1.  Coordinates are x = (double)(x * scale), the product
 * in float32 as sttode_kde_nll; everything after that is float64 unless stated.
 * Weights: W = sum_k w_k in sample order, p_k = w_k / W, s2 = sum_k p_k^2 in sample order, P = #{k : w_k > 0}.  A sample with w_k == 0 is not
 * part of the set: its coordinates enter no sum, minimum or rank (they may be NaN).  A row with a negative or non-finite weight or W == 0
 * makes every output of that agent NaN (decided on the device).  Multiplying a row's weights by a power of two changes no bit.
 * ADE_k / FDE_k: bok_select_kernel's float32 values (bok_dist, frames in frame order).  D_k / L_k: the float64 mean-over-frames / last-frame
 * distance to gt; d_ij / l_ij the same between samples i < j (F.pdist order), t_ij = sqrt(sum_t |x_i,t - x_j,t|^2).
 * Per agent, float64 [n], required:
 *   eade = sum p_k D_k, efde = sum p_k L_k;  es_ade = eade - sum_{i<j} p_i p_j d_ij, es_fde = efde - sum_{i<j} p_i p_j l_ij (energy scores;
 *   p = 1/K: sttode_sample_spread's);  apd = 2 sum_{i<j} p_i p_j t_ij / (1 - s2), fpd the same with l_ij (the expected distance between two
 *   different draws; NaN if 1 - s2 <= 0, i.e. P = 1; p = 1/K: sttode_sample_spread's);  neff = 1 / s2.
 * Optional (may be NULL):
 *   kde_nll [n]: per frame m = sum p_k x_k, C = sum p_k (x_k - m)(x_k - m)^T / (1 - s2), Sigma = f^2 C with f = neff^(-1/6),
 *   logpdf = logsumexp_k(log p_k - (y - x_k)^T Sigma^-1 (y - x_k) / 2) - log det(2 pi Sigma) / 2 over the samples with p_k > 0, clipped below
 *   at -20; nll = -mean over frames.  NaN if P < 3 (two points are collinear: det C is rounding noise), or C00 <= 0 or det C <= 0 at some
 *   frame (sums in sample order; sttode_kde_nll's rule).  p = 1/K: sttode_kde_nll.
 *   ade_top / fde_top [n,K] float32: samples ranked by weight, descending, ties to the lower index, zero weights last; column k-1 = the
 *   minimum of ADE / FDE over the k highest-ranked samples (fminf: NaN skipped; a prefix that is all NaN gives +inf below 64 samples, as
 *   sttode_sample_spread); columns beyond P repeat column P.  Equal weights: sttode_sample_spread's ade_at_k / fde_at_k bit for bit.
 *   brier_ade / brier_fde [n]: (double)min_k ADE_k + (1 - p_k*)^2, k* the lowest-index positive-weight sample that attains the float32
 *   minimum (NaN if none does); FDE alike.
 * Refused before any launch or write, naming the entry.  One launch, no atomics, every sum in a fixed order: the same bits on every run, and
 * an agent's values do not depend on the rest of the batch. */
int sttode_weighted_set(const float* pred, const float* weights, const float* gt, int n, int K, int Tf, float scale, double* eade, double* efde,
                        double* es_ade, double* es_fde, double* apd, double* fpd, double* kde_nll, double* brier_ade, double* brier_fde,
                        double* neff, float* ade_top, float* fde_top, void* stream);
/* Multi-modal ground truth over a dataset: MMADE / MMFDE of DLow and its successors (the reference computes nothing like it).
 * Do the K samples of agent i cover the futures that agents with a similar history actually had?
 * pred [n,K,Tf,2], past [n,Tp,2], gt [n,Tf,2] float32; seg_ptr NULL (n_seg = 0: all agents are one segment) or a CSR [n_seg+1] over the
 * agents, int32 on the device (every bound is clamped to [0, n]; an agent that no segment covers keeps only itself).
 * Coordinates are x = (double)(x * scale), the product in float32 as sttode_kde_nll; everything after that is float64; eps is in scaled units.
 *   anchor a_i = P_i[Tp-1];  history vector H_i = (P_i[t] - a_i) for t = Tp-1-h .. Tp-2, h = hist_frames: 2h numbers;
 *   d_hist(i,j) = sqrt(sum (H_i - H_j)^2), summed in frame order, x then y;
 *   S_i = { j in i's segment : d_hist(i,j) <= eps } + { i }.  A NaN in either history makes the comparison false: such an agent keeps only
 *   itself and enters nobody else's set.  j in S_i <=> i in S_j.
 *   translated future of a neighbour: g_j->i[t] = (Y_j[t] - a_j) + a_i, in exactly that order;
 *   D_ade(i,k,j) = (1/Tf) sum_t |X_i,k,t - g_j->i[t]|, frames summed in frame order;  D_fde(i,k,j) = the last frame's term.
 * Per agent [n]:  count = |S_i| (int32, >= 1);
 *   mmade = (1/count) sum over j in S_i, ascending j, of min_k D_ade(i,k,j);  mmfde the same with D_fde (float64).  A sample with a NaN is
 *   skipped in the minimum; if every sample is NaN the minimum is +inf, and it propagates.
 * At eps = 0 with pairwise distinct histories count = 1 and mmade / mmfde are the float64 best-of-K ADE / FDE; with eps huge count is the size
 * of i's segment.
 * ws: a workspace of ws_doubles >= (2h + 2) n doubles (anchors and history vectors, component-major), overwritten.
 * Limits: 1 <= n <= 2^20, 1 <= K <= 64, Tf >= 1, Tp >= 2, 1 <= h <= Tp - 1, eps >= 0 and finite, scale finite, n_seg >= 1 with seg_ptr.
 * Refused before any launch or write, naming the entry.  No atomics, every sum in a fixed order: the same bits on every run, and an agent's
 * values do not depend on the agents outside its segment. */
int sttode_multimodal(const float* pred, const float* past, const float* gt, const int* seg_ptr_or_NULL, int n_seg, int n, int K, int Tp,
                      int Tf, int hist_frames, float scale, double eps, double* ws, long ws_doubles, int* count, double* mmade, double* mmfde,
                      void* stream);

/* Stage-2 latent sampler (sampler.py:47-54): z = b (eps_mode 0) or A*eps + b with eps shared [nz] (1, share_eps) or per agent
 * [n,nz] (2); logvar = log(A^2 + 1e-8).  A, b, z, logvar [n*K, nz] (row = agent*K + k). */
int sttode_sampler_latent(const float* A, const float* b, const float* eps, int eps_mode, float* z, float* logvar, int n, int K,
                          int nz, void* stream);

/* Stage-2 objective, per agent (samplerloss.py:4-20, utils/dist.py:22-30): kld[a] = sum_{k,d} KL(N(mu,logvar) || N(pmu,plogvar))
 * (pmu / plogvar NULL = standard normal); div[a] = mean over the K(K-1)/2 sample pairs of exp(-|m_i - m_j|^2 / scale),
 * motion [n,K,D] (D = 2*Tf).  The caller sums over agents, divides by agent_num, clamps and weights. */
int sttode_sampler_loss(const float* mu, const float* logvar, const float* pmu, const float* plogvar, const float* motion, int n,
                        int K, int nz, int D, float scale, float* kld, float* div, void* stream);

/* Backward of sttode_sampler_loss: upstream g_kld[a], g_div[a] -> dmu, dlogvar [n*K,nz], dmotion [n,K,D]. */
int sttode_sampler_loss_bwd(const float* mu, const float* logvar, const float* pmu, const float* plogvar, const float* motion,
                            const float* g_kld, const float* g_div, int n, int K, int nz, int D, float scale, float* dmu,
                            float* dlogvar, float* dmotion, void* stream);

/* Stage-2 objective with its ground-truth terms, one launch over all agents; an agent's K samples are staged once and
 * serve every term.  Inputs of sttode_sampler_loss, plus gt [n,Tf,2] and mask [n,Tf] (float32; NULL = all ones); motion [n,K,Tf,2],
 * D = 2 Tf.  Limits: n, nz > 0, K > 1, D even, K * D <= 4096, scale > 0; mu, logvar, motion, gt and every output are required.
 * Per agent, float32 [n] (best: int32 [n]):
 *   kld, div    sttode_sampler_loss's, bit for bit (its lane-to-pair assignment and its order of sums).
 *   rec         min_k sum_t (m_t (x_k,t - y_t))^2 = min_k sum_t m_t^2 |x_k,t - y_t|^2: recon_loss (samplerloss.py:23-29) before its
 *               mean over agents; the mask multiplies the difference, as there.
 *   best        the k of that minimum, the smallest on exact ties (an agent masked entirely: K zeros, best 0).
 *   es_ade      (1/K) sum_k D_ade(x_k, y) - ((K-1)/(2K)) pade,  D_ade(u, v) = (1/Tf) sum_t |m_t (u_t - v_t)|, pade the mean of D_ade over
 *               the K(K-1)/2 sample pairs: sttode_sample_spread's energy score at scale 1 without a mask.
 *   es_fde      the same with D_fde(u, v) = |m_Tf-1 (u_Tf-1 - v_Tf-1)| and fpd.
 *   A masked frame (m_t = 0) contributes zero displacement to both halves; the denominators stay Tf.
 * Precision: kld and div float32 as sttode_sampler_loss.  rec and the ground-truth half of the energy scores: float64 differences, norms
 * and sums of the float32 inputs.  The pair half: sqrtf of the float32 dx, dy that the DLow sum forms, summed in float64.
 * Refused before any launch or write, naming the entry.  No atomics, every sum in a fixed order: the same bits on every run. */
int sttode_sampler_objective(const float* mu, const float* logvar, const float* pmu, const float* plogvar, const float* motion,
                             const float* gt, const float* mask, int n, int K, int nz, int D, float scale, float* kld, float* div,
                             float* rec, int* best, float* es_ade, float* es_fde, void* stream);

/* Backward of sttode_sampler_objective: upstream g_kld, g_div, g_rec, g_es_ade, g_es_fde [n] (each may be NULL = zero) -> dmu, dlogvar
 * [n*K,nz] and ONE summed dmotion [n,K,Tf,2]; every element is written (zeros where nothing flows).  The same limits and refusals.
 *   dmu, dlogvar, and dmotion with g_rec = g_es_* = 0: sttode_sampler_loss_bwd's, bit for bit.
 *   rec:     g_rec 2 m_t (m_t (x_best,t - y_t)) to the one sample `best`, recomputed by the forward's code.
 *   energy:  ce_t (u(x_k,t - y_t) / K - sum_{j != k} u(x_k,t - x_j,t) / K^2),  u(v) = m_t (m_t v) / |m_t v|,
 *            ce_t = g_es_ade / Tf + (t == Tf-1 ? g_es_fde : 0).
 *   u(v) = 0 where |m_t v| = 0 (torch's subgradient of a 2-norm at 0; what sttode_sampler_loss_bwd does for pdist). */
int sttode_sampler_objective_bwd(const float* mu, const float* logvar, const float* pmu, const float* plogvar, const float* motion,
                                 const float* gt, const float* mask, const float* g_kld, const float* g_div, const float* g_rec,
                                 const float* g_es_ade, const float* g_es_fde, int n, int K, int nz, int D, float scale, float* dmu,
                                 float* dlogvar, float* dmotion, void* stream);

/* Scene-level (joint) forms of the stage-2 objective's sample terms (csrc/sampler_joint.hip; added within ABI version 15).
 * Inputs of sttode_sampler_objective, plus seg_ptr [S+1] (int32, device): CSR segment offsets in the convention of sttode_joint_select.
 * Segment g is the agents seg_ptr[g] .. seg_ptr[g+1]-1 (n_g of them): a scene of a batch, the one scene of a step, one NBA game.
 * x_{a,k} is agent a's sample k; sample k of all agents of g is one scene future.  np = K (K-1) / 2, D = 2 Tf.
 *   kld [n]     per agent, sttode_sampler_loss's, bit for bit.
 *   div [S]     joint DLow, unmasked over all D coordinates:  d2_g(i,j) = (1/n_g) sum_{a in g} |x_{a,i} - x_{a,j}|^2,
 *               div_g = (1/np) sum_{i<j} exp(-d2_g(i,j) / scale).  The per-agent squared distance is the float32 sum that
 *               sampler_loss_kernel forms; the sum over agents is float64, in agent order.
 *   rec [S]     J_g(k) = sum_{a in g} sum_t (m_{a,t} (x_{a,k,t} - y_{a,t}))^2 in float64; rec_g = J_g(best_g).
 *   best [S]    int32: the first k that minimises J_g(k); ties go to the lowest k by (ov < bv || (ov == bv && oi < bi)).  A NaN never wins
 *               a comparison, best_g is always a valid column, and the NaN stays in its segment's values.
 *   es [S]      joint energy score on the scene's RMS displacement
 *               R_g(U,V) = sqrt( (1/(n_g Tf)) sum_{a in g} sum_t |m_{a,t} (u_{a,t} - v_{a,t})|^2 ):
 *               es_g = (1/K) sum_k R_g(x_k, y) - (1/K^2) sum_{i<j} R_g(x_i, x_j)   (the 1/K^2 double sum of E R(X,y) - E R(X,X')/2).
 *               With n_g = 1 and Tf = 1 this is sttode_sampler_objective's es_fde.
 * An empty segment writes NaN values and index 0.  seg_ptr's contents are the caller's responsibility; every segment is clamped to [0, n].
 * workspace: ws_bytes >= sttode_sampler_objective_joint_ws(n, K, S) bytes on the device, aligned to 8 bytes, overwritten; it carries
 * nothing from one call to the next.  The entries allocate nothing and read nothing back (they can be captured into a graph).
 * Limits: those of sttode_sampler_objective (n, nz > 0, K > 1, D even, K * D <= 4096, scale > 0), S >= 1; mu, logvar, motion, gt, seg_ptr,
 * workspace and every output are required.  Refused before any launch or write, naming the entry.
 * Precision: kld and the per-agent DLow sums float32; every sum over agents, the differences to the ground truth, R, J and the energy sums
 * float64; outputs float32.  No atomics; every sum's order is a function of the segment's size alone: the same bits on every run, and a
 * segment's outputs depend neither on the other segments nor on its place in the batch. */
/* The workspace size in bytes for n agents, K samples, S segments; negative for arguments the entries refuse. */
long long int sttode_sampler_objective_joint_ws(int n, int K, int S);
int sttode_sampler_objective_joint(const float* mu, const float* logvar, const float* pmu, const float* plogvar, const float* motion,
                                   const float* gt, const float* mask, const int* seg_ptr, int S, int n, int K, int nz, int D, float scale,
                                   void* workspace, long ws_bytes, float* kld, float* div, float* rec, int* best, float* es, void* stream);

/* Backward of sttode_sampler_objective_joint: upstream g_kld [n], g_div, g_rec, g_es [S] (each may be NULL = zero) -> dmu, dlogvar
 * [n*K,nz] (sttode_sampler_loss_bwd's, bit for bit) and ONE summed dmotion [n,K,Tf,2]; every element is written.  The same limits and
 * refusals; the segment's values are recomputed into the workspace by the forward's code.  For agent a of segment g, sample i, frame t:
 *   div:  g_div[g] (1/np) sum_{j != i} exp(-d2_g(i,j) / scale) (-2 / (scale n_g)) (x_{a,i} - x_{a,j})
 *   rec:  g_rec[g] 2 m (m (x_{a,i,t} - y_{a,t})) on i = best_g only, for every agent of g
 *   es:   g_es[g] [ m (m (x_{a,i,t} - y_{a,t})) / (K n_g Tf R_g(x_i, y)) - sum_{j != i} m (m (x_{a,i,t} - x_{a,j,t})) / (K^2 n_g Tf R_g(x_i, x_j)) ]
 * R = 0 contributes a zero gradient (the subgradient 0 of a norm at 0, as sttode_sampler_objective_bwd). */
int sttode_sampler_objective_joint_bwd(const float* mu, const float* logvar, const float* pmu, const float* plogvar, const float* motion,
                                       const float* gt, const float* mask, const int* seg_ptr, int S, const float* g_kld,
                                       const float* g_div, const float* g_rec, const float* g_es, int n, int K, int nz, int D, float scale,
                                       void* workspace, long ws_bytes, float* dmu, float* dlogvar, float* dmotion, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training step (csrc/train*.hip, one file per kernel family: index in train.hip): forward-with-tape + backward of STTODENet.forward() (model/STTODE.py:553-568; losses
 * :372-395; what train.py:81-87 drives through total_loss.backward()).  Generic kernels over row-major nn.Parameter storage;
 * gradients are ACCUMULATED into the caller's .grad buffers.  All matrices row-major with explicit leading dimensions.
 * ------------------------------------------------------------------------------------------------ */
/* out[c, i] = mask( act( sum_j X[c / xdiv, j] * Wop[i, j] + bias[i] (+ out[c, i] if accumulate) ) ), c < cols, j < J, i < I.
 * trans = 0: Wop[i, j] = W[i*ldw + j] (nn.Linear forward);  trans = 1: Wop[i, j] = W[j*ldw + i] (input gradient dX = dY W).
 * act: 0 none | 1 relu | 2 tanh | 3 sigmoid.  mask (optional, [cols, ldm]): result zeroed where mask <= 0 (relu backward). */
int sttode_tlinear(const float* X, long ldx, int xdiv, const float* W, long ldw, int trans, const float* bias, const float* mask,
                   long ldm, float* Y, long ldy, int cols, int J, int I, int act, int accumulate, void* stream);
/* Y[c, 0:I] = act(W X[c] + tab[c / tdiv] (+ bias)): nn.Linear on cat(shared, own) with the shared part's product -- identical for tdiv
 * consecutive columns -- handed over as a table tab [cols / tdiv, ldt].  The decoder MLPs' layer 1 (model/utils.py:86-95 on
 * cat(past_feature_rep, z, state), model/STTODE.py:71-75,322-328): tab = W1[:, pf] pf + b1 per AGENT (n rows), W = W1[:, z | state] per
 * trajectory -- half the layer's products, the inference chain's layer-1 split in the training step. */
int sttode_tlinear_tab(const float* X, long ldx, const float* W, long ldw, const float* bias, const float* tab, long ldt, int tdiv, float* Y,
                       long ldy, int cols, int J, int I, int act, void* stream);
/* dW[n, k] += sum_c dY[c, n] * X[c / xdiv, k];  db[n] += sum_c dY[c, n] (db may be NULL).  Deterministic: fixed column splits,
 * partials in scratch (scratch_floats capacity; NULL = single split). */
int sttode_twgrad(const float* dY, long ldy, const float* X, long ldx, int xdiv, float* dW, long ldw, float* db, int cols, int N,
                  int K, float* scratch, long scratch_floats, void* stream);
/* Backward of one nn.Linear: dX[c, 0:Kdx] = mask(sum_n dY[c, n] W[n, 0:Kdx] (+ dX)) and dW += dY^T X, db += sum_c dY, in ONE
 * launch when cols <= 1024 (the launch-bound training regime; dX must not alias dY or X), otherwise sttode_tlinear + sttode_twgrad. */
int sttode_tlinear_bwd(const float* dY, long ldy, const float* W, long ldw, const float* mask, long ldm, float* dX, long lddx,
                       int Kdx, int accumulate, const float* X, long ldx, int xdiv, float* dW, long ldgw, float* db, int cols, int N,
                       int K, float* scratch, long scratch_floats, void* stream);
/* Batch sizes (cols > 2048) split a weight gradient's reduction over the columns; the partial sums are added into dW / db by a reduction
 * launch.  sttode_twgrad_defer(1, buf, floats): from now on the partial sums are bump-allocated from buf (device memory nothing else
 * writes) and the reductions run as ONE launch per 16 gradients -- or earlier: buf full, a destination that is already pending, another
 * stream.  sttode_twgrad_defer(0, NULL, 0): run what is pending (on the stream of the gradients that queued it), back to a reduction per
 * gradient; sttode_twgrad_defer(-1, NULL, 0): forget what is pending (error paths).  sttode_twgrad_flush(): run what is pending, keep the
 * mode.  Host-side state of the calling thread; a training step brackets its backward pass with defer(1) / defer(0) (sttode_amd/training.py). */
int sttode_twgrad_defer(int on, float* buf, long floats);
int sttode_twgrad_flush(void);
/* Grouped launches: between sttode_tgemm_group(1) and sttode_tgemm_group(0) the batch-size products (cols > 2048) of sttode_tlinear,
 * sttode_twgrad and sttode_tlinear_bwd are queued and leave as ONE launch (at most 4 products per launch; a fifth starts the next).  The
 * caller promises that the products of a group do not depend on each other and do not write the same output; calls below the batch
 * size launch at once as usual.  sttode_tgemm_group(-1): forget what is queued (error paths).  Host-side state of the calling thread (a group is
 * opened, filled and closed by one thread).  Also queued inside a group: scene-size layers (cols <= 1024) of sttode_tlinear /
 * sttode_tlinear_bwd, element-wise pieces (sttode_train_ewise) and a second sttode_ttrunk_fwd. */
int sttode_tgemm_group(int on);
/* inp0 / inp1 [n K1, ld] (inp1 may be NULL), row (a, k): columns 0..pfw-1 = pf[a] (rows of ldpf floats; pfw = 2 hidden_dim), pfw..pfw+zd-1 =
 * qz[a] for k = 0, else eps[a, k - 1] (eps [n (K1 - 1), zd]): the layer-1 input prefix of the decompose blocks (model/STTODE.py:322-331,
 * 553-566).  pfw, zd multiples of 4 (128 / 32 at the reference's defaults). */
int sttode_decoder_inputs(float* inp0, float* inp1, long ld, const float* pf, long ldpf, const float* qz, const float* eps, int n, int K1,
                          int pfw, int zd, void* stream);
/* dst[r, 0:width] = src[(r / div) % mod, 0:width] (repeat_interleave: div = K; per-frame tables: mod = T). */
int sttode_rows_copy(float* dst, long ldd, const float* src, long lds, int rows, int width, int div, int mod, void* stream);
/* dst[a, f] (+)= sum_{k<K} src[a*K + k, f]  (backward of repeat_interleave). */
int sttode_rows_reduce(float* dst, long ldd, const float* src, long lds, int rows_out, int width, int K, int accumulate, void* stream);
/* Element-wise pieces, op codes: 0 p0=p1*p2 | 1 p0+=f0*p1 | 2 gate backward (dout=p0, tanh out p1, sigmoid out p2 -> p3, p4;
 * hypertransformer.py:81-83) | 3 p0=relu(p1+f0*p2) (Euler step + relu, ode_demo.py:188,228) | 4 its backward (dout p0, out p1 ->
 * p3 += d, p4 = f0*d) | 5 rsample z=mu+eps*exp(logvar/2) (model/STTODE.py:89-93; params p1 [rows,2*i0], eps p2) | 6 p0=p1*(p2>0) |
 * 7 p0=f0 | 8 rsample backward (dz p0, params p1, eps p2 -> dparams p3 +=) | 9 p0[c,d] += p1[c / K, d % 2] (row length i0,
 * K = f0: "+ cur_location", model/STTODE.py:343-344) | 10 p0=p1*(1-p2^2) (tanh backward from its output) | 11 stage-2 latent
 * backward (sampler.py:51-53): dz p0, dlogvar p1, A p2, eps p3 -> dA p4 = dz*eps + dlogvar*2A/(A^2+1e-8); i0 = nz*4 + eps_mode,
 * f0 = K*nz | 12 p0[c,d] = p1 + p2 (+ p3[c / K, d % 2]) (row length i0, K = f0: sum of the blocks' outputs + cur_location) |
 * 13 op 4 on dout = cat(dx0 | dode), rows of p0 with leading dimension i0 (64 features): d = dode*(out p1 > 0), p3 = dx0 + d, p4 = f0*d |
 * 14 p0 = f0*p0 (+ p1) | 15 p0[r, c] += f0*p1[r*ld + c], c < width (width = i0 & 0xffff, ld = i0 >> 16).
 * Inside a group (sttode_tgemm_group) up to four pieces leave as one launch. */
int sttode_train_ewise(int op, float* p0, const float* p1, const float* p2, float* p3, float* p4, long count, int i0, float f0,
                       void* stream);
/* y = LayerNorm(x + r) over D = hidden_dim features (32 / 64 / 128; hypertransformer.py:146,151); saves xhat [rows,D], rstd [rows]. */
int sttode_add_ln_fwd(const float* x, const float* r, const float* gamma, const float* beta, float* y, float* xhat, float* rstd,
                      int rows, int D, void* stream);
/* LayerNorm backward: dsum = grad wrt (x + r); dgamma, dbeta += ; scratch >= 64 * 2 D floats. */
int sttode_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dsum, float* dgamma,
                  float* dbeta, int rows, int D, float* scratch, long scratch_floats, void* stream);
/* nn.GRU cell, gate order r|z|n (model/STTODE.py:68): gi [m rows, ld ldgi] = W_ih e_t + b_ih, gh [m,288] = W_hh h + b_hh;
 * tape [m,384] = r, z, n, gh_n.  hprev NULL = zero state. */
int sttode_gru_cell_fwd(const float* gi, long ldgi, const float* gh, const float* hprev, float* hnew, float* tape, int m, void* stream);
/* dh [m,96] (grad wrt h') -> dgi (ld ldgi), dgh [m,288], dhprev = dh * z (the W_hh^T dgh term is added by sttode_tlinear). */
int sttode_gru_cell_bwd(const float* dh, const float* tape, const float* hprev, float* dgi, long ldgi, float* dgh, float* dhprev,
                        int m, void* stream);
/* The same over the WHOLE sequence in one launch (columns are independent): gi [m*Tp,288] (row = col*Tp + t), H [(Tp+1),m,96]
 * with H[0] = 0 on entry (H[t+1] = h_t written), tapes [Tp,m,384].  W_hh fragments stay in registers across the steps. */
int sttode_gru_seq_fwd(const float* gi, const float* Whh, const float* bhh, float* H, float* tapes, float* hfinal, long ldhf, int m,
                       int Tp, void* stream);   /* hfinal (optional): the final state also goes to rows of ldhf floats */
/* Whole BPTT in one launch: dh_last [m,96] = grad wrt the final state -> dgi [m*Tp,288], dgh [Tp,m,288]
 * (dh_{t-1} = dh_t * z_t + dgh_t W_hh is carried in registers / LDS). */
int sttode_gru_seq_bwd(const float* dh_last, long lddh, const float* tapes, const float* H, const float* Whh, float* dgi, float* dgh,
                       int m, int Tp, void* stream);
/* conv1d(2->32,k3,pad1)+relu (model/STTODE.py:65) on x = xa[c / adiv] - xb[c] ([m,T,2], xb optional); saves x; e [m,T,32]. */
int sttode_conv_fwd(const float* xa, int adiv, const float* xb, const float* w, const float* b, float* x, float* e, int m, int T,
                    void* stream);
/* de (already relu-masked) -> dx [m,T,2] (optional), dw [32,2,3] +=, db [32] += (deterministic: per-WG partials in scratch,
 * >= 256*224 floats, then one ordered pass). */
int sttode_conv_bwd(const float* de, const float* x, const float* w, float* dx, float* dw, float* db, int m, int T, float* scratch,
                    long scratch_floats, void* stream);
/* Backward of the geodesic self-attention (hyptransformerlib.py:191-300, scores untransposed :261-265): qkv [L*Nb, 3 D] (q|k|v,
 * row = l*Nb + slot; D = 8 head_dim), dO [L*Nb, D] (grad wrt the merged-head output before out_proj) -> dqkv [L*Nb, 3 D].
 * head_dim 4 / 8 / 16; L (4 head_dim + 4) floats of LDS (L <= 1137 at head_dim 8). */
int sttode_mhgsa_attn_bwd(const float* qkv, const float* dO, float* dqkv, int L, int Nb, int head_dim, void* stream);
/* Backward of sttode_mhgsa_attn (head_dim 8) for any rows x cols: R, C, V, dO in the operands' layout of the forward call (dO laid out like
 * `out`, strides os_*) -> dR, dC, dV in the layouts of R, C, V (overwritten, not accumulated).  Both orientations of the drop-ins' mhgsa:
 * L != S (R = q, C = k) and the untransposed L == S form (R = k, C = q).  Gradients through the clamp follow torch.clamp (bounds inclusive),
 * through both normalisations and both scales.  One workgroup per (slot, head), deterministic; rows (2 head_dim + 3) + cols (2 head_dim + 1)
 * floats of LDS must fit 64 KiB (rows = cols <= 455). */
int sttode_mhgsa_attn_rc_bwd(const float* R, const float* C, const float* V, const float* dO, float* dR, float* dC, float* dV, int rows,
                             int cols, int Nb, long rs_seq, long rs_b, long cs_seq, long cs_b, long vs_seq, long vs_b, long os_seq,
                             long os_b, float rscale, float cscale, void* stream);
/* torch.optim.Adam's step (train.py:122 constructs it, :66,87 call it) for ALL parameters in ONE launch: items = DEVICE array of n records
 * {float* p, float* m, float* v, long goff, long numel, long chunk0} (48 bytes each): parameter, first / second moment, the gradient's offset
 * in floats from gbase, element count, first 1024-element chunk (ascending from 0; `chunks` = their total).  step = t >= 1 (bias
 * corrections 1 - beta^t).  m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2; p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 -
 * beta2^t) + eps); weight_decay adds weight_decay * p to g first (torch's L2 form).  amsgrad / maximize: not built (the caller falls back). */
int sttode_adam_step(const void* items, int n, long chunks, const float* gbase, double lr, double beta1, double beta2, double eps,
                     double weight_decay, long step, void* stream);
/* Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) and a non-finite guard in front of the optimizer step
 * (train.py:64-66,85-87: backward, then optimizer.step(); the reference carries a detect_grad_nan, core/utils.py:268-272, and never calls
 * it), on the device with no host round trip.  Added within ABI version 14.
 * One param group: the table of sttode_adam_step (the p / m / v pointers are read by sttode_adam_step_guarded only) and the group's Adam
 * hyper-parameters; step = the t the group's next update would have had no step ever been skipped (0: no Adam scalars wanted). */
typedef struct SttodeGradGroup {
    const void* items; int n; long chunks; const float* gbase;
    double lr, beta1, beta2; long step;
} SttodeGradGroup;
#define STTODE_GRAD_MAX_GROUPS 16
/* The device state block: STTODE_GRAD_STATE_WORDS 32-bit words owned by the caller, zeroed once (or with `applied` preset).
 *   [0] total_norm (float)  [1] coef (float)  [2] apply (int)  [3] applied (int)  [4] skipped (int)  [5..7] reserved
 *   [8 + 2 g], [9 + 2 g]: lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t) of group g (float), t = step - skipped */
#define STTODE_GRAD_STATE_WORDS 40
/* groups: HOST array of ngroups <= STTODE_GRAD_MAX_GROUPS records.  One launch per group writes the sum of squares of each 1024-element
 * chunk to partials (DEVICE, partials_len >= the groups' chunks together; fixed summation order, no atomics: repeatable bit for bit, NaN /
 * Inf propagate); one workgroup then sums them in double and writes the state block: total_norm, coef = min(1, max_norm / (total_norm +
 * 1e-6)) (max_norm > 0; 0 = no clipping: coef 1), apply = 0 when skip_nonfinite and the norm is NaN / Inf (then `skipped` counts the step,
 * else `applied`), and each group's two scalars: sttode_adam_step's own values for t = step while nothing was ever skipped, else
 * recomputed on the device for t = step - skipped. */
int sttode_grad_norm(const SttodeGradGroup* groups, int ngroups, float* partials, long partials_len, double max_norm, int skip_nonfinite,
                     void* state, void* stream);
/* sttode_adam_step on g * coef, with coef, apply and the two scalars of slot `group` read from the state block sttode_grad_norm wrote in
 * front of it on the stream; apply == 0: nothing is stored.  coef == 1 and nothing skipped: sttode_adam_step's result bit for bit. */
int sttode_adam_step_guarded(const void* items, int n, long chunks, const float* gbase, double beta1, double beta2, double eps,
                             double weight_decay, const void* state, int group, void* stream);
/* g *= coef in place for every tensor of the table (the second half of a stand-alone clip_grad_norm_); coef == 1: nothing is stored. */
int sttode_grad_scale(const void* items, int n, long chunks, float* gbase, const void* state, void* stream);
/* out[0] = scale * sum (pred - target)^2 (calculate_loss_pred / _recover, :372-376,384-388); dpred optional. */
int sttode_loss_sqerr(const float* pred, const float* target, long count, float scale, float* out, float* dpred, void* stream);
/* KL term (:378-382, utils/dist.py:26-29), params [rows,2*zd].  scene_ptr NULL: out[0] = clamp_min(sum KL / denom, min_clip).
 * scene_ptr [S+1] (a batch of independent scenes in one step): out[0] = sum_s clamp_min(sum_{a in s} KL_a / N_s, min_clip), i.e. the
 * sum of the per-scene objectives (what accumulating S reference steps gives).  scratch >= max(S, 1) floats. */
int sttode_loss_kl(const float* params, const int* scene_ptr, int S, int rows, int zd, float denom, float min_clip, float* out,
                   float* dparams, float* scratch, void* stream);
/* Best-of-K term (calculate_loss_diverse :390-395); pred [n,K,D], target [n,D], K <= 64.  scene_ptr NULL: mean over the n agents;
 * with scene_ptr / agent_scene: sum over scenes of the per-scene means.  scratch >= n floats. */
int sttode_loss_diverse(const float* pred, const float* target, const int* scene_ptr, const int* agent_scene, int n, int K, int D,
                        float* out, float* dpred, float* scratch, void* stream);
/* Training step, forward of ONE encoder trunk with its tape in one launch (PastEncoder / FutureEncoder trunk, model/STTODE.py:214-236 /
 * :276-300, hypertransformer.py:134-153, ode_demo.py:188,228) for attention length 1 (scene batches: softmax over one key == 1).
 * `ptrs`: table of STT_TT_COUNT device pointers -- the trunk's parameters in their row-major nn.Parameter storage, the inputs, and every
 * tensor sttode_amd/training.py's trunk_bwd reads.  feat: row stride ld_feat, [0,64) = ftraj_input, [64,128) = ODE encoder output.
 * T <= 12 (LDS); otherwise, and for attention groups > 1, the caller runs the layer-by-layer entry points. */
enum SttodeTrunkPtr {
    STT_TT_FC1_W, STT_TT_FC1_B, STT_TT_POS_W, STT_TT_POS_B, STT_TT_FC2_W, STT_TT_FC2_B, STT_TT_FC3_W, STT_TT_FC3_B, STT_TT_INPROJ_W,
    STT_TT_INPROJ_B, STT_TT_OUT_W, STT_TT_OUT_B, STT_TT_INFO_W, STT_TT_INFO_B, STT_TT_GATE_W, STT_TT_GATE_B, STT_TT_LN1_W, STT_TT_LN1_B,
    STT_TT_L1_W, STT_TT_L1_B, STT_TT_L2_W, STT_TT_L2_B, STT_TT_LN2_W, STT_TT_LN2_B,
    STT_TT_ENC_IN /* [n,T,4] */, STT_TT_LAST /* int32 [n] */, STT_TT_PE /* [>=T,64] */, STT_TT_DROP /* [n*T,64] keep mask / keep, or NULL */,
    STT_TT_POSIN /* [n*T,128] */, STT_TT_TP /* [n*T,64] */, STT_TT_H3IN /* [n,68] */, STT_TT_FEAT, STT_TT_XC /* [n,64] */,
    STT_TT_QKV /* [n,192] */, STT_TT_AO, STT_TT_TT, STT_TT_SS, STT_TT_H, STT_TT_XH1 /* [n,64] each */, STT_TT_RS1 /* [n] */,
    STT_TT_F1 /* [n,1024] */, STT_TT_XH2, STT_TT_RS2, STT_TT_ODE,
    STT_TT_ATTN /* [n,64]: phase 2 only -- the attention output (before out_proj) of sttode_mhgsa_attn over the forward-call batch */, STT_TT_COUNT
};
/* phase 0: the whole trunk (attention length 1).  Attention over the forward-call batch (the NBA branch): phase 1 = up to the in-projection
 * (writes qkv, xc, feat[:, :64]), then sttode_mhgsa_attn(_groups) as its own launch, then phase 2 = from ptrs[STT_TT_ATTN] on. */
int sttode_ttrunk_fwd(const void* const* ptrs, int count, int n, int T, long ld_feat, float ode_time, int phase, void* stream);
/* Training through a non-default encoder integrator (ABI 9; csrc/train_ode.hip): the linear stage combinations of the fixed-grid program
 * (Euler, 3/8-rule 'rk4', classical RK4 on a uniform grid, oracle.sttode_ref.ode_integrate_ref) and of its discrete adjoint.  A job writes
 * out[r, c] = sum_t c[t] v[t][r ld[t] + c] over rows x width (masked to 0 where mask[r ld_mask + c] <= 0 when mask != NULL) and, when
 * relu_out != NULL, also relu_out[r ld_relu + c] = max(out, 0).  jobs = HOST array of `count` <= STT_ODE_MAX_JOBS records.  One launch. */
#define STT_ODE_MAX_TERMS 6
#define STT_ODE_MAX_JOBS 4
typedef struct SttodeOdeCombine {
    const float* v[STT_ODE_MAX_TERMS];
    long ld[STT_ODE_MAX_TERMS];
    float c[STT_ODE_MAX_TERMS];
    float* out;
    long ld_out;
    float* relu_out;
    long ld_relu;
    const float* mask;
    long ld_mask;
    int nterms;
    int rows;
} SttodeOdeCombine;
int sttode_ode_combine(const void* jobs, int count, int width, void* stream);
/* The fixed-grid program's coefficients (sttode_amd/odestages.py TABLEAU): stage i reads y + h sum_j a[4 i + j] k_j, the step is
 * y + h sum_i b[i] k_i; stages 1 (Euler) or 4. */
typedef struct SttodeOdeProgram {
    int stages;
    int steps;
    float h;
    float a[16];
    float b[4];
} SttodeOdeProgram;
/* Integration forward of `trunks` <= 2 encoder trunks in ONE launch, attention length 1, T <= 12 (as sttode_ttrunk_fwd): each trunk's
 * layers up to ftraj_input exactly as sttode_ttrunk_fwd phase 1 (ptrs: trunks x STT_TT_COUNT pointers, as there), then the whole stage
 * program of `prog` (HOST) inside the kernel.  Writes the stage inputs ys[t] [steps * stages * n[t], 64] (stage j's rows at j n[t]),
 * y_T into yT[t] [n[t], 64] and relu(y_T) into feat[:, 64:128]. */
int sttode_ttrunk_ode_fwd(const void* const* ptrs, int count, int trunks, const int* n, const int* T, const long* ld_feat, float* const* ys,
                          float* const* yT, const void* prog, void* stream);
/* Per-stage dX chain of the same program's backward (attention length 1), one launch for up to STT_ODE_MAX_JOBS / 2 trunks: per row, f is
 * recomputed from the stage input y, dk = sum of the `kb` terms (the stage-combination adjoint; kb.out unused), back-propagated through
 * LN2, linear2^T, the relu mask, linear1^T, LN1, the gate, temporal_info / temporal_gate^T, out_proj^T and in_proj(v)^T into dy; when
 * next.out != NULL also next.out = dy + sum of the `next` terms (the gradient wrt the step's start state, on its first stage).  Writes
 * every linear layer's X and dY columns (attn = v, ao, h, f1 [n,1024], dsum2, df1 [n,1024], du, dv, dao, dattn) and the LayerNorm
 * parameter-gradient rows ln [n,256] = [dk xhat2 | dk | dh xhat1 | dh] for the deferred weight-gradient pass; no cross-row reductions.
 * w: in_proj_weight, in_proj_bias, out_proj w / b, temporal_info w / b, temporal_gate w / b, norm1 w / b, linear1 w / b, linear2 w / b,
 * norm2 w / b (row-major nn.Parameter storage).  jobs = HOST array of `count` records. */
typedef struct SttodeOdeStageBwd {
    const float* w[16];
    const float* y;
    SttodeOdeCombine kb;
    float* dy;
    SttodeOdeCombine next;
    float* attn;
    float* ao;
    float* h;
    float* f1;
    float* dsum2;
    float* df1;
    float* du;
    float* dv;
    float* dao;
    float* dattn;
    float* ln;
    int n;
} SttodeOdeStageBwd;
int sttode_ode_stage_bwd(const void* jobs, int count, void* stream);

/* The four terms of forward()'s objective (:372-395,553-568) and all their gradients for ONE decoder pass over K1 = 1 + K samples per
 * agent (sample 0: decoded from the posterior draw, enters the prediction / recover terms; samples 1..K: the prior draws, best-of-K):
 * pred [n,K1,D], rec [n,K1,Dp], fut [n,D], past [n,Dp], qzp [n,2*zd] -> out[0..4] = (mse, recover, kl, diverse as the three entry
 * points above compute them, then their sum = total_loss), dpred [n,K1,D], drec [n,K1,Dp] (zero rows for samples 1..K), dqzp [n,2*zd].  Two launches.
 * scratch_floats >= 3 n + S with a scene CSR, 4 n without one (3 n + max(S, n) floats cover both; refused otherwise): [3][n] per-agent
 * partial sums, then one KL value per scene, or without a CSR one KL row sum per agent. */
int sttode_loss_objective(const float* pred, const float* rec, const float* fut, const float* past, const float* qzp,
                          const int* scene_ptr, const int* agent_scene, int S, int n, int K1, int D, int Dp, int zd, float scale_mse,
                          float scale_rec, float kl_denom, float min_clip, float* out, float* dpred, float* drec, float* dqzp,
                          float* scratch, long scratch_floats, void* stream);
/* The same objective, gradients for the LIVE decoder columns only.  Of an agent's K1 trajectory columns only sample 0 (posterior draw: the
 * mse and recover terms, model/STTODE.py:553-560) and the best of samples 1..K (loss_diverse takes the min over K, :390-395: torch's min
 * passes its gradient to the selected sample alone) receive a gradient; the decoder treats columns independently, so the backward pass of
 * every other column is exactly zero.  -> dpred2 [n,2,D], drec2 [n,2,Dp] (row 1 zero), best [n] (1..K: which sample row 1 is), out / dqzp
 * and scratch (3 n + max(S, n) floats) as above.  The reference's autograd multiplies through the zero rows; a backward pass over 2 n instead of K1 n columns is the same
 * gradient (tests/test_gpu_parity.py::test_training_step_vs_reference_*). */
int sttode_loss_objective_live(const float* pred, const float* rec, const float* fut, const float* past, const float* qzp,
                               const int* scene_ptr, const int* agent_scene, int S, int n, int K1, int D, int Dp, int zd, float scale_mse,
                               float scale_rec, float kl_denom, float min_clip, float* out, float* dpred2, float* drec2, float* dqzp,
                               int* best, float* scratch, long scratch_floats, void* stream);
/* The same objective with the SCENE-LEVEL (joint) best-of-K term in the diverse slot (beyond the reference): the min over the
 * K = K1 - 1 prior samples is taken outside the sum over a segment's agents, so every agent of a segment selects the same sample.
 * Segments are runs of consecutive agents: with scene_ptr [S+1] the scenes (seg_len must be 0); with scene_ptr NULL runs of seg_len agents
 * (seg_len >= 1 divides n; seg_len == n: one scene; NBA: the agents of one game).  J_g(k) = sum_{a in g} sum_d (fut[a,d] - pred[a,k,d])^2,
 * k*_g = the first k in 1..K minimising J_g (ties to the lowest k), out[3] = sum_g w_g J_g(k*_g) with w_g the weight sttode_loss_objective gives
 * an agent of g (1 / agents of the scene with a CSR, 1 / n otherwise), out[4] = ((out[0] + out[1]) + out[2]) + out[3].
 * -> dpred2 [n,2,D] (row 1 = 2 (pred[a,k*_g] - fut[a]) w_g), drec2 [n,2,Dp] (row 1 zero), best [n] = k*_g(a) (1..K), seg_best [G] = k*_g
 * (optional, NULL: not written; G = S or n / seg_len); out[0..2], dqzp and row 0 of both gradients are sttode_loss_objective_live's bit for
 * bit, and with one-agent segments so is everything else.  Per-agent sums in fp32, the sum over a segment's agents in double in a fixed
 * order: results repeat bit for bit and a segment's best / gradients depend on its own agents only.  Two launches.
 * Refused before any launch: a null pointer (best included), K1 outside 2..65, n, D, Dp or zd <= 0, scene_ptr without S > 0 and agent_scene,
 * no scene_ptr and kl_denom <= 0, seg_len != 0 with scene_ptr, seg_len < 1 or not a divisor of n without, scratch_floats < 3 n + S with
 * a CSR or < 4 n without one ([3][n] per-agent slots -- the third holds a segment's value in its first agent's slot and zeros -- then the KL
 * values, as above). */
int sttode_loss_objective_joint(const float* pred, const float* rec, const float* fut, const float* past, const float* qzp,
                                const int* scene_ptr, const int* agent_scene, int S, int n, int K1, int D, int Dp, int zd, float scale_mse,
                                float scale_rec, float kl_denom, float min_clip, float* out, float* dpred2, float* drec2, float* dqzp,
                                int* best, int seg_len, int* seg_best, float* scratch, long scratch_floats, void* stream);
/* The joint term alone (the counterpart of sttode_loss_diverse): pred [n,K,D] (the K prior samples), target [n,D], 1 <= K <= 64, segments
 * as above (with scene_ptr, agent_scene [n] is required: the number of scenes is agent_scene[n-1] + 1).  out[0] = the term, bit for bit
 * out[3] of sttode_loss_objective_joint on the same samples; dpred [n,K,D] optional (zero rows but the selected one), best [n] optional
 * (1..K).  scratch >= n floats.  Two launches. */
int sttode_loss_diverse_joint(const float* pred, const float* target, const int* scene_ptr, const int* agent_scene, int n, int K, int D,
                              int seg_len, float* out, float* dpred, int* best, float* scratch, void* stream);
/* ... and the rows of the forward pass's tape for those columns: items = HOST array of `count` <= 32 records {const float* src; float* dst;
 * long src_plane; long dst_plane; int row; int outer;} (40 bytes): src is `outer` planes (src_plane floats apart) of [n K1] rows of `row`
 * floats, dst `outer` planes (dst_plane apart) of [2 n] rows; dst row 2 a + j = src row a K1 + (j ? best[a] : 0).  One launch. */
int sttode_live_rows_gather(const void* items, int count, const int* best, int n, int K1, void* stream);
/* forward() returns its four loss terms as Python floats (model/STTODE.py:568: four `.item()`, each a synchronisation with the END of the
 * queue).  Inside a replayed step the values exist after the forward half: sttode_publish_values (one launch, capturable) copies
 * vals [n <= 64] (DEVICE) into host_vals [n] (pinned HOST memory, device-accessible), increments *dev_seq (DEVICE, zero before the first
 * launch) and stores the new count into *host_seq (pinned HOST); sttode_wait_value spins on the host until *host_seq == (unsigned)want (0) or
 * timeout_s seconds have passed (non-zero) -- no stream, no event: whatever is queued behind the publishing launch keeps running. */
int sttode_publish_values(const float* vals, int n, float* host_vals, unsigned* dev_seq, unsigned* host_seq, void* stream);
int sttode_wait_value(const unsigned* host_seq, long want, double timeout_s);

/* ------------------------------------------------------------------------------------------------
 * Stand-alone manifold op library (not on the model's data flow; op-level parity).
 * Row ops, x/y/out [rows,d] (scalar results: out [rows]); op codes (hyptorch/pmath.py unless noted):
 *  0 project :98-103   1 lambda_x :128-129  2 mobius_add :171-177  3 dist :205-208   4 dist0 :231-234
 *  5 expmap :268-277 (y = u)  6 expmap0 :300-304  7 logmap :334-339  8 logmap0 :365-368  9 p2k :440-442
 * 10 k2p :445-447  11 lorenz_factor :450-469  12 Oblique.proj (core/manifolds/oblique.py:15-16)
 * 13/14 internal halves of mobius_matvec / poincare_mean.
 * ------------------------------------------------------------------------------------------------ */
int sttode_pmath_rowop(int op, const float* x, const float* y, float* out, float* out2, int rows, int d, float c, void* stream);
/* which: 0 tanh (clamp 15, pmath.py:11-12), 1 artanh (:16-22), 2 arsinh (:51-55), 3 d artanh/dx at the clamped input
 * (Artanh.backward :25-27), 4 d arsinh/dx (Arsinh.backward :57-60) */
int sttode_pmath_scalar(int which, const float* x, float* out, long n, void* stream);
/* RiemannianGradient.backward (pmath.py:39-45): out[r,:] = g[r,:] * (1 - c |x_r|^2)^2 / 4. */
int sttode_pmath_riemannian_grad(const float* x, const float* g, float* out, int rows, int d, float c, void* stream);
/* mobius_matvec (pmath.py:399-408): m [O,d], x [rows,d] -> out [rows,O]; workspaces mx_ws [rows,O], xnorm_ws [rows]. */
int sttode_pmath_matvec(const float* m, const float* x, float* mx_ws, float* xnorm_ws, float* out, int rows, int d, int O, float c,
                        void* stream);
/* which: 0 dist_matrix (pmath.py:482-493) out [P,R]; 1 _mobius_addition_batch (:416-427) out [P,R,d];
 * 2 _hyperbolic_softmax (:430-437) with x = P [C,d], y = X [B,d], A [C,d] -> out [B,C]. */
int sttode_pmath_pair(int which, const float* x, const float* y, const float* A, float* out, int P, int R, int d, float c,
                      void* stream);
/* poincare_mean over dim 0 (pmath.py:472-479): x [rows,d] -> out [d]; workspaces yl_ws [rows,d], lam_ws [rows]. */
int sttode_pmath_mean(const float* x, float* yl_ws, float* lam_ws, float* out, int rows, int d, float c, void* stream);
/* Backward passes (csrc/pmath_grad.hip; added within ABI version 14).  Gradients are WRITTEN, not accumulated.
 * Row ops 0..11: g is the upstream gradient, [rows,d] for vector results and [rows] for the scalar results (lambda_x, dist, dist0,
 * lorenz_factor); gx [rows,d]; gy [rows,d] is required exactly for the four two-operand ops (mobius_add, dist, expmap, logmap) and must be
 * NULL otherwise.  Op 12 (Oblique.proj) and the internal codes 13/14 are refused.  One launch, no workspace; only x, y, g are read. */
int sttode_pmath_rowop_bwd(int op, const float* x, const float* y, const float* g, float* gx, float* gy, int rows, int d, float c, void* stream);
/* mobius_matvec backward: m [O,d], x [rows,d], g [rows,O] -> gx [rows,d], gm [O,d] (zeroed here first).  Workspaces mx_ws [rows,O] (x m^T is
 * recomputed into it by sttode_tlinear; afterwards it holds the split sums of sttode_twgrad), gmx_ws [rows,O] (gradient with respect to
 * x m^T).  gxn_ws [rows] is not a workspace of the computation but an unused OUTPUT: the gradient with respect to |x| per row is written to
 * it once and read by nothing (the row kernel puts that term into gx itself); it must not be NULL.  _project's branch is chosen by a float64
 * test on the recomputed x m^T and can differ from the forward kernel's fp32 choice for a row within fp32 rounding of the maximal norm.  gx = gmx m + gxn x / |x| (sttode_tlinear, trans = 1), gm = gmx^T x (sttode_twgrad).
 * Not inside a sttode_tgemm_group bracket.  DEVIATION from the reference: a row with x m^T == 0 gets a zero gradient (the reference: NaN). */
int sttode_pmath_matvec_bwd(const float* m, const float* x, const float* g, float* mx_ws, float* gmx_ws, float* gxn_ws, float* gx, float* gm,
                            int rows, int d, int O, float c, void* stream);
/* dist_matrix backward: x [P,d], y [R,d], g [P,R] -> gx [P,d], gy [R,d].  Two launches (one wave per x row, one wave per y row), sums in a
 * fixed order: bitwise repeatable, no atomics. */
int sttode_pmath_dist_matrix_bwd(const float* x, const float* y, const float* g, float* gx, float* gy, int P, int R, int d, float c,
                                 void* stream);
/* _hyperbolic_softmax backward (added within ABI version 14): X [B,d], A [C,d], P [C,d], g [B,C] -> gX [B,d], gA [C,d],
 * gP [C,d], all written.  coef_ws holds 6 B C doubles: g times the partial of the logit with respect to each of the pair's six scalars,
 * written once per pair and then read by one wave per X row and one wave per class row, partners in index order: bitwise repeatable, no
 * atomics.  A zero row of A is outside the domain (the reference gives NaN). */
int sttode_pmath_hsoftmax_bwd(const float* X, const float* A, const float* P, const float* g, double* coef_ws, float* gX, float* gA, float* gP,
                              int B, int C, int d, float c, void* stream);
/* Feature clipping of hyptorch/nn.py's ToPoincare(clip_r=r): out = x min(1, r / (|x| + 1e-5)) over rows of x [rows,d], and its backward
 * pass g [rows,d] -> gx [rows,d]; r > 0. */
int sttode_pmath_clip(const float* x, float* out, int rows, int d, float r, void* stream);
int sttode_pmath_clip_bwd(const float* x, const float* g, float* gx, int rows, int d, float r, void* stream);
/* The curvature on the device, and its gradient (csrc/pmath.hip, csrc/pmath_grad.hip; added within ABI version 15).
 * c_dev points to ONE float on the device that the kernels read: no host read of a trainable curvature, and the calls can be captured.
 * Forward: the argument lists of sttode_pmath_rowop (ops 0..11 only), sttode_pmath_matvec and sttode_pmath_pair with c_dev in place of c;
 * for *c_dev == v the results are bitwise those of the float form at v.  A NULL c_dev is refused; the VALUE cannot be checked on the
 * host: a curvature that is not positive gives NaN, not a refusal. */
int sttode_pmath_rowop_c(int op, const float* x, const float* y, float* out, float* out2, int rows, int d, const float* c_dev, void* stream);
int sttode_pmath_matvec_c(const float* m, const float* x, float* mx_ws, float* xnorm_ws, float* out, int rows, int d, int O,
                          const float* c_dev, void* stream);
int sttode_pmath_pair_c(int which, const float* x, const float* y, const float* A, float* out, int P, int R, int d, const float* c_dev,
                        void* stream);
/* Backward: the float forms' argument lists with c_dev in place of c, plus gc_ws -- one double per row of the op (rows; rows; P; B), each
 * row's share of dL/dc -- and gc [1], the gradient of the curvature: WRITTEN (not accumulated) by one workgroup that adds gc_ws in a fixed
 * order; no atomics, bitwise repeatable.  Tensor-gradient outputs may be NULL where nothing needs them: gx and gy of the row ops (gy must
 * still be NULL for a one-operand op); gx, gm, gxn_ws of mobius_matvec (gmx_ws too when gx and gm are both NULL; mx_ws is always needed);
 * gx, gy of dist_matrix; gX, and gA with gP, of _hyperbolic_softmax, whose coef_ws holds SEVEN planes here, 7 B C doubles.  Where they
 * are given their values are bitwise those of the float form at c = *c_dev. */
int sttode_pmath_rowop_bwd_c(int op, const float* x, const float* y, const float* g, float* gx, float* gy, int rows, int d, const float* c_dev,
                             double* gc_ws, float* gc, void* stream);
int sttode_pmath_matvec_bwd_c(const float* m, const float* x, const float* g, float* mx_ws, float* gmx_ws, float* gxn_ws, float* gx, float* gm,
                              int rows, int d, int O, const float* c_dev, double* gc_ws, float* gc, void* stream);
int sttode_pmath_dist_matrix_bwd_c(const float* x, const float* y, const float* g, float* gx, float* gy, int P, int R, int d,
                                   const float* c_dev, double* gc_ws, float* gc, void* stream);
int sttode_pmath_hsoftmax_bwd_c(const float* X, const float* A, const float* P, const float* g, double* coef_ws, float* gX, float* gA,
                                float* gP, int B, int C, int d, const float* c_dev, double* gc_ws, float* gc, void* stream);
/* Oblique.dist (core/manifolds/oblique.py:36-43): p1 [nb,n1,d], p2 [nb,n2,d] -> acos(clamp(p2 p1^T)) [nb,n2,n1]. */
int sttode_oblique_dist(const float* p1, const float* p2, float* out, int nb, int n1, int n2, int d, void* stream);
/* Opt-in gradients through poincare_mean and the Oblique entry points (csrc/pmath.hip, csrc/pmath_grad.hip; added within
 * ABI version 15).
 * poincare_mean (pmath.py:472-479) at a general shape: x [outer,R,inner,d] -> out [outer,inner,d], the mean over R, with no permuted copy
 * (pmath.py:475-479 with dim any but the last).  Workspaces yl_ws as x, lam_ws [outer,R,inner].  One block per group runs the sums of
 * sttode_pmath_mean in its order: a group's result is bitwise that of sttode_pmath_mean on its rows.  The curvature is *c_dev when c_dev is
 * given (one float on the device, unchecked), else c (> 0, finite).  klein [outer,inner,d] and lsum [outer,inner] (each may be NULL)
 * receive the Klein mean before k2p and the sum of the Lorentz factors. */
int sttode_pmath_mean_seg(const float* x, float* yl_ws, float* lam_ws, float* out, float* klein, float* lsum, int outer, int R, int inner,
                          int d, float c, const float* c_dev, void* stream);
/* poincare_mean backward: g [outer,inner,d] -> gx as x, WRITTEN.  Workspaces gS_ws [outer inner d] and gL_ws [outer inner] doubles: a group
 * stage (one wave per group: the Klein sums recomputed in float64 from x, then k2p's vector-Jacobian product) and a row stage (one wave per
 * row).  Two launches, no atomics, bitwise repeatable.  The _c form reads the curvature from c_dev and WRITES its gradient gc [1] in a third
 * launch, from gc_ws: outer R inner + outer inner doubles (each row's share, then each group's); its gx may be NULL. */
int sttode_pmath_mean_bwd(const float* x, const float* g, double* gS_ws, double* gL_ws, float* gx, int outer, int R, int inner, int d, float c,
                          void* stream);
int sttode_pmath_mean_bwd_c(const float* x, const float* g, double* gS_ws, double* gL_ws, float* gx, int outer, int R, int inner, int d,
                            const float* c_dev, double* gc_ws, float* gc, void* stream);
/* Oblique.proj backward (oblique.py:15-16): gp = (g - <g,y> y) / |p| with y = p / |p|, rows of [rows,d]; a zero row gives NaN as the
 * forward does. */
int sttode_oblique_proj_bwd(const float* p, const float* g, float* gp, int rows, int d, void* stream);
/* Oblique.dist backward (oblique.py:36-43): g [nb,n2,n1] -> gp1 [nb,n1,d], gp2 [nb,n2,d] (either may be NULL, not both).  The clamp at
 * +-(1 - 1e-4) has torch.clamp's gradient: zero where the un-clamped inner product is strictly outside.  One launch per output, row sums in
 * a fixed order. */
int sttode_oblique_dist_bwd(const float* p1, const float* p2, const float* g, float* gp1, float* gp2, int nb, int n1, int n2, int d,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * Riemannian optimisation (csrc/manifold.hip): the manifold interface of core/manifolds/base.py as row operations, and
 * Riemannian Adam / SGD over every manifold parameter of a param group in one launch.  Added within ABI version 14.  sttode_manifold_rowop_bwd is the row ops' backward pass.
 * ---------------------------------------------------------------------------------------------- */
enum SttodeManifold { STT_MF_EUCLIDEAN = 0, STT_MF_OBLIQUE, STT_MF_POINCARE, STT_MF_COUNT };
enum SttodeManifoldOp { STT_MOP_PROJ_TAN = 0, STT_MOP_EXPMAP, STT_MOP_PTRANSP, STT_MOP_INNER, STT_MOP_RETR, STT_MOP_RETR_TRANSP, STT_MOP_COUNT };
enum SttodeRiemannianRule { STT_RULE_ADAM = 0, STT_RULE_SGD, STT_RULE_COUNT };
/* One op on the rows of a, b, w [rows,d] (one wave per row, float64 row sums):
 *   PROJ_TAN     (p, u)     out = egrad2rgrad(p, u): Oblique u - <p,u> p (its proj_tan), ball u (1 - c |p|^2)^2 / 4, Euclidean u
 *   EXPMAP       (p, u)     out = expmap(u, p), no projection; Oblique keeps the reference's branch at |u| = 1e-4 (zero u: p / |p|)
 *   PTRANSP      (x, y, u)  out = ptransp(x, y, u): Oblique proj_tan(u, y), ball gyr[y, -x] u lambda_x / lambda_y
 *   INNER        (p, u, v)  out [rows] = inner_p(u, v); w == NULL: v = u
 *   RETR         (x, u)     out = retr(x, u): Oblique expmap renormalised, ball project(expmap)
 *   RETR_TRANSP  (x, u, v)  out = y = retr(x, u), out2 = ptransp(x, y, v)
 * c: the ball's curvature magnitude (> 0, finite); ignored by the other manifolds.  Operands an op does not take may be NULL. */
int sttode_manifold_rowop(int op, int manifold, const float* a, const float* b, const float* w, float* out, float* out2, int rows, int d,
                          float c, void* stream);
/* The backward pass of the six row ops on every manifold (added within ABI version 15; core/manifolds/oblique.py:15-27,
 * :60-74 and the ball's operations above, differentiated as the forward evaluates them).  g: the upstream gradient, [rows,d] ([rows] for
 * INNER); g2: RETR_TRANSP's second upstream gradient (of out2), NULL for every other op; for RETR_TRANSP either of g, g2 may be NULL,
 * meaning zero.  ga, gb, gw [rows,d]: the gradients of the operands, WRITTEN; each may be NULL (not all), gw is ignored by the ops that take
 * no third operand.  Branches differentiate as taken: Oblique expmap below |u| = 1e-4 as proj(p + u); the ball's retraction through
 * project's clip, chosen by the forward kernel's own fp32 test.  One launch, no workspace, no atomics, bitwise repeatable. */
int sttode_manifold_rowop_bwd(int op, int manifold, const float* a, const float* b, const float* w, const float* g, const float* g2, float* ga,
                              float* gb, float* gw, int rows, int d, float c, void* stream);
/* One optimiser step of every parameter of a DEVICE table.  A wave steps one WAVE SLOT: one row of d > 32 elements, two rows of d <= 32,
 * four rows of d <= 16; a parameter takes ceil(rows / rows per slot) slots.  A table row is STTODE_RIEMANNIAN_ITEM_WORDS 8-byte words:
 * parameter, state buffer 1 (Adam exp_avg [rows,d]; SGD momentum_buffer or NULL for momentum 0), state buffer 2 (Adam exp_avg_sq [rows];
 * SGD unused), gradient, d, rows, first wave slot (ascending from 0; total_slots = the slots of all parameters), manifold code, c (a
 * double), element count (rows d; a plain parameter of the SGD rule is cut into rows of d elements, the last may be short).  Per row, with g += weight_decay x
 * and r = egrad2rgrad(x, g):
 *   ADAM  m = beta1 m + (1 - beta1) r; v = beta2 v + (1 - beta2) inner_x(r, r); y = retr(x, -lr (m / (1 - beta1^t)) / (sqrt(v / (1 -
 *         beta2^t)) + eps)); m = ptransp(x, y, m); x = y.  t >= 1: the step count.  t == 0 with tstate (DEVICE, one double): the count
 *         is kept on the device, incremented by a one-thread launch in front of the step (a captured step replays correctly); a call with
 *         t >= 1 and tstate writes t there.
 *   SGD   buf = momentum buf + r (with a buffer); y = retr(x, -lr buf); buf = ptransp(x, y, buf); x = y.  beta1, beta2, eps, t unused.
 * No atomics, no host synchronisation, no allocation; bitwise repeatable. */
#define STTODE_RIEMANNIAN_ITEM_WORDS 10
int sttode_riemannian_step(int rule, const void* table, int nrows_table, long total_slots, double lr, double beta1, double beta2,
                           double eps, double weight_decay, double momentum, long t, void* tstate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gromov delta-hyperbolicity (hyptorch/delta.py:12-35).  Stand-alone analysis, not on the model's data flow.
 * ------------------------------------------------------------------------------------------------ */
/* scipy.spatial.distance_matrix of T row samples (delta.py:29-31): X [rows,d] row-major; idx [T,n] int32 row indices into X (NULL: the rows
 * as given, then T == 1 and n == rows); dist [T,n,n] (dist_floats >= T n^2) gets sqrt(sum_k (x_i - x_j)^2) in fp32, k in order for every
 * pair -- bitwise symmetric, exact zero diagonal; diam [T] gets each try's maximum (delta.py:32; zeroed on `stream` first).  An idx entry
 * outside [0, rows) reads nothing and gives NaN distances and a NaN diameter.  1 <= n <= 32768, 1 <= T <= 65535, d >= 1. */
int sttode_delta_dist(const float* X, int rows, int d, const int* idx, int T, int n, float* dist, long dist_floats, float* diam, void* stream);
/* *floats = the workspace sttode_delta_hyp needs for T tries of n points, in floats (either path).  Host only. */
int sttode_delta_workspace(int T, int n, long* floats);
/* delta_hyp (delta.py:12-23) of T matrices at once: dist [T,n,n] (dist_floats >= T n^2; any finite values, symmetry not required) ->
 * delta [T] = max_ij (max_k min(A[i,k], A[k,j]) - A[i,j]) with A[i,j] = 0.5f * ((D[0,j] + D[i,0]) - D[i,j]), all in fp32 (min / max exact):
 * delta, not delta / diam.  symmetric = 1 only when every D is bitwise symmetric (sttode_delta_dist's output is): then only the tiles
 * j-block >= i-block run, with the same result.  ws [ws_floats >= sttode_delta_workspace(T, n)] holds per-tile maxima; two launches. */
int sttode_delta_hyp(const float* dist, int T, int n, long dist_floats, int symmetric, float* ws, long ws_floats, float* delta, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Oversample and reduce: Lloyd k-means of M sampled futures per agent to K representatives.  Added WITHIN ABI version 14:
 * one new export, nothing else changed, so a binding built for 14 keeps working.
 * ------------------------------------------------------------------------------------------------ */
/* pred [R,n,K_in,Tf,2] fp32, round-major: R stacked outputs [n,K_in,Tf,2] of inference.  Sample m = r K_in + k of agent a starts at
 * (((r n + a) K_in + k) Tf) 2; M = R K_in; R = 1 is the familiar [n,M,Tf,2].  With x[m] agent a's sample m, a point of R^(2 Tf), and
 * t0 = from_frame:
 *     c_0 = init
 *     for i = 1 .. iters:
 *         label_i[m] = argmin_k sum_{t >= t0} |x[m,t] - c_{i-1}[k,t]|^2        (the lowest k on exact ties)
 *         c_i[k]     = mean of x[m] over {m : label_i[m] = k}, ALL frames       (c_{i-1}[k] if that set is empty)
 *     centroids [n,K,Tf,2] fp32 = c_iters, labels [n,M] int32 = label_iters, counts [n,K] int32: counts[k] = |{m : label_iters[m] = k}|
 * from_frame = 0 clusters whole trajectories, from_frame = Tf - 1 endpoints; the representatives are full mean trajectories either way, and
 * counts / M are their weights.  This is scipy.cluster.vq.kmeans2(x[:, sliced], init[:, sliced], iter=iters, minit='matrix') for the labels
 * and the sliced code book, including the rule that an empty cluster keeps its centroid.
 * init_mode 0 ('first'): the agent's samples 0 .. K-1 (i.i.d. draws: Forgy initialisation); 1 ('maximin'): sample 0, then K-1 times the
 * sample whose squared distance (same frame slice) to its nearest chosen sample is largest, the lowest index on ties; 2: the caller's
 * init [n,K,Tf,2].  init is non-NULL exactly in mode 2.
 * Arithmetic: fp32 throughout; distances are direct sums of squared differences over the slice in coordinate order (never the expanded
 * |x|^2 - 2 x.c + |c|^2 form); a cluster's members are added in sample order and the sum is divided by the count; no floating-point
 * atomics.  Two runs give the same bits, and an agent's result depends on its own samples only (the same bits alone or inside any batch).
 * The loop ends early once an iteration changes no label (further iterations would reproduce the same bits).  Non-finite inputs: outputs
 * unspecified, labels still in [0, K), nothing read or written out of bounds.
 * One workgroup per agent; the agent's samples are staged in LDS when they fit (about 4 (2 Tf) (M + 2 K) + 5 M bytes within 160 KiB: M = 1000
 * at Tf = 12 does), otherwise every pass re-reads them from global memory / L2 with the same result.
 * Limits, refused before anything is launched or written: n >= 1, 1 <= K <= 64, K <= M <= 4096, 1 <= Tf <= 200, 0 <= from_frame < Tf,
 * 1 <= iters <= 1000, init_mode in {0, 1, 2}. */
int sttode_reduce_samples(const float* pred, int n, int R, int K_in, int Tf, int K, int iters, int from_frame, int init_mode,
                          const float* init, float* centroids, int* labels, int* counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Oversample and reduce whole scenes: Lloyd k-means in which a sample is one future of a whole segment.  Added WITHIN ABI
 * version 15: one new export, nothing else changed, so a binding built for 15 keeps working.
 * ------------------------------------------------------------------------------------------------ */
/* pred [R,n,K_in,Tf,2] fp32, round-major, exactly as for sttode_reduce_samples; M = R K_in.  seg_ptr [S+1] int32 on the device, the CSR of
 * sttode_joint_select: segment s (a scene, an NBA game) holds the agents seg_ptr[s] .. seg_ptr[s+1]-1 (every bound is clamped to [0, n] and
 * to its predecessor on the device; agents outside every segment keep whatever their centroids held).  Sample m of a segment is the scene
 * future made of sample m of each of its A agents, a point of R^(A 2 Tf); all agents of a segment share one label per sample and one count
 * per cluster.  With x[a,m] agent a's sample m and t0 = from_frame, per segment s:
 *     c_0 = init
 *     for i = 1 .. iters:
 *         d_a(m,k)      = sum_{t >= t0} |x[a,m,t] - c_{i-1}[a,k,t]|^2                 (fp32)
 *         D(m,k)        = sum over the segment's agents a, in order, of (double) d_a(m,k)
 *         label_i[s,m]  = argmin_k D(m,k)                                             (the lowest k on exact ties)
 *         c_i[a,k]      = mean of x[a,m] over {m : label_i[s,m] = k}, ALL frames      (c_{i-1}[a,k] if that set is empty, for every agent alike)
 *     centroids [n,K,Tf,2] fp32 = c_iters, labels [S,M] int32 = label_iters, counts [S,K] int32: counts[s,k] = |{m : label_iters[s,m] = k}|
 * Representative k of a segment is then one coherent scene future, and counts / M are the weights of the scene futures.
 * init_mode 0 ('first'): scene futures 0 .. K-1, i.e. every agent's samples 0 .. K-1; 1 ('maximin'): scene future 0, then K-1 times the
 * scene future whose distance D (same slice, float64 sum over the agents of the fp32 per-agent squared distances) to its nearest pick is
 * largest, the lowest index on ties; 2: the caller's init [n,K,Tf,2].  init is non-NULL exactly in mode 2.
 * Arithmetic: d_a(m,k) has the bits sttode_reduce_samples computes (an fma chain over the slice in coordinate order from 0, direct
 * differences); the sum over agents is float64 in segment order; a cluster's members are added in sample order starting from the first
 * member and the sum is divided by the count, in fp32; no floating-point atomics.  Hence a CSR of one-agent segments gives the bits of
 * sttode_reduce_samples (centroids, labels, counts); two runs give the same bits; a segment's outputs are the same bits alone, with segments
 * appended behind it or with agents put in front of it.  The loop ends early once an iteration changes no label.  An empty segment gets
 * labels 0 and counts (M, 0, ..) and touches no centroid.  Non-finite inputs: outputs unspecified, labels still in [0, K), nothing read or
 * written out of bounds.
 * One workgroup per segment for the whole loop; the centroids live in the output array, labels and counts in LDS; no workspace.
 * Limits, refused before anything is launched or written: n >= 1, S >= 1, 1 <= K <= 64, K <= M <= 4096, 1 <= Tf <= 200, 0 <= from_frame < Tf,
 * 1 <= iters <= 1000, init_mode in {0, 1, 2}, no NULL among pred, seg_ptr, centroids, labels, counts.  Nothing is refused for the size of a
 * segment: it may be all n agents. */
int sttode_reduce_scenes(const float* pred, int n, int R, int K_in, int Tf, int K, int iters, int from_frame, int init_mode,
                         const float* init, const int* seg_ptr, int S, float* centroids, int* labels, int* counts, void* stream);
/* Scores of a whole oversampled set (csrc/large_set.hip; added within ABI version 15): the M = R K_in futures per agent that
 * sttode_reduce_samples / sttode_reduce_scenes cluster, scored themselves -- best-of-M and its prefixes, joint best-of-M, KDE NLL at the
 * literature's sample count, and the pair statistics of the set -- where sttode_best_of_k_select, sttode_joint_select, sttode_kde_nll and
 * sttode_sample_spread hold one sample per lane and keep refusing K > 64.
 * pred is round-major [R,n,K_in,Tf,2] float32 (R stacked outputs of inference: sample m = r K_in + k; R = 1 is a plain [n,M,Tf,2]), gt
 * [n,Tf,2] float32; coordinates are scaled as in the entry each one mirrors.
 * Limits of all three, refused by name before anything is launched or written: n >= 1, R >= 1, K_in >= 1, 1 <= M <= 4096, 1 <= Tf <= 200, no
 * NULL among the required pointers.  M <= 64 is taken: there the values tie to the entries above.
 * Sum order, wherever a sum runs over samples or pairs: thread tid of 256 adds its own terms in ascending order (samples tid, tid + 256, ...),
 * the 64 lanes of a wave are added by the xor tree 32, 16, .. 1, the four waves in wave order, the workgroups of an agent in workgroup order.
 * No atomics: two runs give the same bits, and an agent's or a segment's values do not depend on the rest of the batch.
 * sttode_large_select:
 *   ADE(a,m) / FDE(a,m): the float32 values bok_select_kernel computes for a sample (bok_dist, frames added in frame order, / Tf).
 *   ade / fde [n] = min over m; best_ade_idx / best_fde_idx [n] = the lowest m that attains it; miss [n] = fde > miss_threshold (strictly).
 *   A value wins only by being smaller (<) than the best so far, which starts at +inf with index 0: a NaN never wins, and an agent with no
 *   finite sample gets +inf and index 0 (not bok_select_kernel's NaN).  For finite inputs and M <= 64 the outputs are
 *   sttode_best_of_k_select's bit for bit.
 *   ks: nk <= 16 values ON THE HOST, strictly ascending in [1, M] (nk = 0: ks, ade_at, fde_at NULL): ade_at / fde_at [n,nk], column i = the
 *   minimum over the first ks[i] samples in m order, by the same rule.
 *   seg_ptr [S+1] (device CSR, bounds clamped to [0, n]; NULL: no joint outputs, the four seg_* NULL, S ignored): per segment and sample the
 *   sum over the segment's agents of ADE(a,m), in double, in agent order, / agent count; seg_jade [S] = its minimum over m as float32,
 *   seg_jade_idx [S] = the lowest m that attains it (compared as doubles); seg_jfde / seg_jfde_idx alike.  Any segment size.  An empty
 *   segment gets NaN and -1, one without a finite sample +inf and 0; a one-agent segment gives the agent's ade / fde / indices bitwise.
 *   The joint outputs need ws, ws_bytes >= sttode_large_select_ws(n, M) bytes on the device (the per-sample values, overwritten).
 *   Optional (NULL): best_ade_idx, best_fde_idx, miss.
 * sttode_large_kde_nll (M >= 3): sttode_kde_nll's definition over the M samples -- float64 on x = (double)(x * scale), per frame the
 *   unbiased covariance, Scott's factor M^(-1/6), the closed-form inverse and determinant, a two-pass logsumexp, clipped below at -20, NaN
 *   where C00 <= 0 or det C <= 0 at some frame; nll [n] float64 = -mean over frames.  The four sums over samples per frame in the order above.
 * sttode_large_spread (M >= 2; div_scale > 0 and finite): sttode_sample_spread's apd / fpd / pade / dlow and, with gt (else es_ade = es_fde
 *   = NULL), es_ade / es_fde over the M (M-1) / 2 pairs, float64 [n], same definitions and arithmetic.  The pairs are tiles of 64 x 64
 *   samples (ib <= jb, row order) dealt to G = min(tiles, 64) workgroups per agent, tile g, g + G, ...; a thread adds its 4 x 4 pairs of a
 *   tile in row order.  ws: ws_bytes >= sttode_large_spread_ws(n, M) bytes on the device (the workgroups' partial sums, overwritten).
 * The two size queries return bytes, or -1 with the error set. */
long long int sttode_large_select_ws(int n, int M);
int sttode_large_select(const float* pred, const float* gt, int n, int R, int K_in, int Tf, float scale, float miss_threshold, const int* ks,
                        int nk, const int* seg_ptr, int S, void* ws, long ws_bytes, float* ade, float* fde, int* best_ade_idx,
                        int* best_fde_idx, unsigned char* miss, float* ade_at, float* fde_at, float* seg_jade, float* seg_jfde,
                        int* seg_jade_idx, int* seg_jfde_idx, void* stream);
int sttode_large_kde_nll(const float* pred, const float* gt, int n, int R, int K_in, int Tf, float scale, double* nll, void* stream);
long long int sttode_large_spread_ws(int n, int M);
int sttode_large_spread(const float* pred, const float* gt, int n, int R, int K_in, int Tf, float scale, double div_scale, void* ws,
                        long ws_bytes, double* apd, double* fpd, double* pade, double* dlow, double* es_ade, double* es_fde, void* stream);
/* Latent sets (csrc/latents.hip; added within ABI version 15): per agent a set of M = R K points of N(0, I) in zdim
 * dimensions, placed rather than drawn independently -- what inference(z=), inference_async(z=) and inference_reduced(z=) take.
 * z [R][n K][zdim] float32, row = agent K + k: set index m of an agent lives at round m / K, column m % K.  bits: NULL, or int32 of the same
 * shape: the 32-bit integer x behind every drawn value, 0 where no value was drawn (the centre row, the mirrored rows).
 * Integer stage, for agent a = first_agent + local index, drawn point j, dimension d (32-bit wrap-around arithmetic):
 *   s(a, d) = Philox4x32-10(key = seed, counter = [a_lo, a_hi, d >> 2, 0])[d & 3]
 *   kind 0 (Sobol): x = XOR over the set bits b of gray(j) = j ^ (j >> 1) of dirs[d 30 + b] << 2; dirs [zdim][30] on the device: the 30-bit
 *     direction numbers of the sequence (sttode_amd/latents.py uploads torch.quasirandom.SobolEngine(zdim).sobolstate), then
 *     scramble 0: x as is (point 0 is the corner u ~ 0 of every dimension, z ~ -6.34: for checks only);
 *     scramble 1 (random digital shift): x ^ s(a, d);
 *     scramble 2 (nested uniform scrambling by hash): brev(h(brev(x), s(a, d))), h the Laine-Karras hash in Burley's form (JCGT 2020):
 *       x += s, x ^= x 0x6c50b47c, x ^= x 0xb82f1e52, x ^= x 0xc7afe638, x ^= x 0x8d22f6e6 -- every step triangular in the bits, so the
 *       net properties of the sequence are kept exactly.
 *   kind 1 (random): x = Philox4x32-10(key = seed, counter = [a_lo, a_hi, d >> 2, 1 + j])[d & 3]; scramble is ignored, dirs may be NULL.
 * Value stage, in float64: u = (x + 0.5) 2^-32; truncate = t > 0: u <- Phi(-t) + u (Phi(t) - Phi(-t)), evaluated as 0.5 + (u - 0.5) w with
 *   w = Phi(t) - Phi(-t) = erf(t / sqrt 2) -- the same number, since Phi(-t) + w / 2 = 0.5, and the form that keeps the digits of a value near
 *   the mode; z = float32(Phi^-1(u)) (AS241 PPND16 on u - 0.5, which is exact), clamped to +-t when truncated.  |z| <= 6.34.
 * Set composition, c = center, B = M - c: without antithetic set index c + j is drawn point j (j < B); with it H = ceil(B / 2) points are
 *   drawn, index c + j is z_j and index c + H + j is -z_j (j < B - H); with center index 0 is the zero vector, the prior mode.
 * Limits, refused by name before anything is launched or written: z non-NULL; n >= 1; K, R >= 1 and M = R K <= 65536; 1 <= zdim <= 1024;
 *   first_agent >= 0; kind 0 or 1; scramble 0, 1 or 2; antithetic, center 0 or 1; truncate 0, or finite and >= 0.01; dirs non-NULL for
 *   kind 0; center needs M >= 2.
 * One launch on `stream`: no workspace, no atomics, two runs give the same bits, and an agent's rows depend on (seed, a) only -- the rows
 * of agents 5..8 drawn with first_agent = 5 are rows 5..8 of a draw of 130 agents. */
int sttode_latent_set(float* z, int* bits, const unsigned* dirs, int n, int K, int R, int zdim, long long first_agent,
                      unsigned long long seed, int kind, int scramble, int antithetic, int center, float truncate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Native forward pipeline: one call enqueues STTODENet.inference (model/STTODE.py:574-623) end to end.
 * ------------------------------------------------------------------------------------------------ */
typedef struct SttodeModel SttodeModel;

/* order of the packed-weight pointer table handed to sttode_model_create (sttode_amd/packing.py names) */
enum SttodeWeight {
    STT_W_FC1P, STT_W_FC1B, STT_W_POSP, STT_W_PEB, STT_W_FC2P, STT_W_FC2B, STT_W_FC3P, STT_W_FC3B, STT_W_FC3LAST, STT_W_INP,
    STT_W_INB, STT_W_OUTP, STT_W_OUTB, STT_W_INFOP, STT_W_INFOB, STT_W_GATEP, STT_W_GATEB, STT_W_LN1W, STT_W_LN1B, STT_W_L1P,
    STT_W_L1B, STT_W_L2P, STT_W_L2B, STT_W_LN2W, STT_W_LN2B,
    STT_W_B0_CONVP, STT_W_B0_CONVB, STT_W_B0_WIHP, STT_W_B0_WHHP, STT_W_B0_GBIAS, STT_W_B0_XWA, STT_W_B0_XB1, STT_W_B0_YWA,
    STT_W_B0_YB1, STT_W_B0_STREAM,
    STT_W_B1_CONVP, STT_W_B1_CONVB, STT_W_B1_WIHP, STT_W_B1_WHHP, STT_W_B1_GBIAS, STT_W_B1_YWA, STT_W_B1_YB1, STT_W_B1_STREAM,
    STT_W_CHAIN_POOL, STT_W_CHAIN_PROG, STT_W_CHAIN_CONSTS, STT_W_G0_POOL, STT_W_G0_PROG, STT_W_G0_CONSTS,
    STT_W_CHAINB3_POOL, STT_W_CHAINB3_PROG,   /* exploratory bf16-split stream of the fused launch (packing.chain_stream_b3) */
    STT_W_ROLE32_POOL, STT_W_ROLE32_PROG_SCENES, STT_W_ROLE32_PROG_NBA, STT_W_ROLE32_CONSTS_SCENES,
    STT_W_ROLE32_CONSTS_NBA,                  /* throughput-form per-agent roles of the lagged launch (packing.role_stream, round 4) */
    STT_W_COUNT
};

/* workspace buffers (offsets in floats from sttode_workspace_layout) */
enum SttodeBuffer {
    STT_B_SCENE_ORIG, STT_B_AGENT_SCENE, STT_B_XPAD, STT_B_ENC_IN, STT_B_CUR, STT_B_ORIG, STT_B_LAST, STT_B_G, STT_B_QKV,
    STT_B_ATTN, STT_B_PF, STT_B_STATE0, STT_B_A0X, STT_B_A0Y, STT_B_A1Y, STT_B_DBUF, STT_B_YBUF, STT_B_STATE1, STT_B_QUEUE, STT_B_FLAGS /* tile flags of the fused launch */,
    STT_B_ODE /* [6][n][64]: state, k1..k4, scratch of the multi-stage integrator with attention groups > 1 */, STT_B_COUNT
};

/* pipeline stages reported by sttode_timing_read */
enum SttodeStage {
    STT_STAGE_FRONTEND, STT_STAGE_EMBED, STT_STAGE_ATTN, STT_STAGE_POST, STT_STAGE_GRU0, STT_STAGE_LINEAR, STT_STAGE_MLP0,
    STT_STAGE_GRU1, STT_STAGE_MLP1, STT_STAGE_CHAIN, STT_STAGE_AGENTS /* encoder + block-0 GRU in one launch (scene batches) */,
    STT_STAGE_FUSED /* per-agent roles + trajectory chain in ONE launch (scene batches, round 3) */, STT_STAGE_COUNT
};

/* STTODENet.__init__ + load_state_dict equivalent for the packed weights (model/STTODE.py:350-366).  The library keeps the weight pointers
 * (the caller keeps the tensors alive) and the model's events; the pipeline's HIP streams are created with the first model of a device
 * and shared by every later model of that device for the life of the process (the runtime deals its few hardware queues to streams
 * round-robin at creation: a later model's own streams could land on the caller's queue and serialise the pipeline). */
int sttode_model_create(SttodeModel** out, const void* const* weights, int count, int Tp, int Tf, int K, int n_chunks0,
                        int n_chunks1);
/* Hand over (or replace) one entry of the weight table after creation.  The two entries of the exploratory bf16-split stream
 * (STT_W_CHAINB3_*) may be NULL at creation and arrive here before sttode_set_mfma_mode(m, 1). */
int sttode_model_set_weight(SttodeModel* m, int index, const void* ptr);
int sttode_model_destroy(SttodeModel* m);
int sttode_workspace_layout(const SttodeModel* m, int n, int S, long* offsets /*[STT_B_COUNT]*/, long* total_floats);
/* ONCE per workspace (after allocation, before its first use by sttode_inference_*): zeroes the hand-off flag words (STT_B_FLAGS) and marks
 * the workspace initialised.  The one-launch scene form (sttode_set_scene_launch) keeps its flag words zero from then on -- the last
 * workgroup of every launch zeroes them again -- so it needs no memset in front of a launch and a captured sttode_inference_scenes replays
 * correctly; launched on a workspace that was never initialised it refuses the flag words it finds: NaN predictions, time-out word 2. */
int sttode_workspace_init(SttodeModel* m, float* workspace, int n, int S, void* stream);
/* per-trajectory stage: 1 = fused chain kernel (sttode_traj_chain), 0 = the three-kernel form (mlp_block0 -> gru_cols -> mlp_block1),
 * -1 = automatic (fused when the batch has >= 128 trajectories per workgroup slot to fill; default). */
int sttode_set_chain(SttodeModel* m, int mode);
/* Calls whose per-trajectory stage takes the fused chain: 1 (default) = the per-agent stage (encoder, block-0 GRU,
 * layer-1 pre-activation tables: PastEncoder.forward model/STTODE.py:214-236, DecomposeBlock.forward :62-75 of block 0) runs as the
 * leading workgroups of the chain launch, trajectory groups wait on one flag per 16-agent tile (attention groups > 1, the NBA branch:
 * the embedding and the attention stay launches in front, the roles start at the post-attention layer); 0 = separate launches on
 * the pipeline's per-agent stream.  Results are bitwise the same in both modes.  Anything else is refused: modes 2-4 (the scene
 * front-end inside the roles, roles interleaved with the groups, five role workgroups per tile) were A/B candidates that lost and are
 * retired (DESIGN_HISTORY.md). */
int sttode_set_fused(SttodeModel* m, int mode);
/* EXPLORATORY, opt-in, never the default (own dtype label in bench.py): 1 = the per-trajectory chain (the three decoder MLPs and block 1's
 * conv + GRU: DecomposeBlock.forward model/STTODE.py:51-77, Decoder.forward :320-347) runs its matrix products as a three-way bf16
 * split on the bf16 matrix cores -- x = hi + mid + lo, six products per k block, fp32 accumulate: fp32-class accuracy, held to the same
 * golden vectors at the same 1e-4 -- instead of fp32 MFMAs; 0 (default, or env STTODE_BF16X3) = fp32 everywhere.  The per-agent stage,
 * the attention and every call below the chain threshold stay fp32 in both modes. */
int sttode_set_mfma_mode(SttodeModel* m, int mode);
/* Fault injection for tests of the in-launch hand-off's give-up path: in fused launches the per-agent role of 16-agent tile `tile` computes
 * its tables but never publishes its flag (-1: off, the default).  The trajectory groups that read that tile then run into the bound of
 * their spin (~1 s), write NaN into their predictions and set the time-out word (workspace buffer STT_B_FLAGS, word [tiles]) -- the
 * launch ends, it never hangs; every other group is unaffected.  The model's host-visible word (sttode_timeout_word) is set as well. */
int sttode_debug_drop_role_flag(SttodeModel* m, int tile);
/* Host staging of one scene for the one-scene-per-call loop (test.py:171-188 -> set_data, model/STTODE.py:397-404): pre [N][2][Tp] and
 * fut [N][2][Tf] (HOST pointers, the loader's layout; fut may be NULL with Tf = 0) are transposed into a pinned ring slot and copied to
 * dev [N*Tp*2 + N*Tf*2] (DEVICE: past [N][Tp][2] followed by future [N][Tf][2]) with one asynchronous copy on `stream`. */
int sttode_stage_scene(const float* pre, const float* fut, int N, int Tp, int Tf, float* dev, void* stream);
/* The same ring for a batch whose host layout IS the device layout (set_data_nba, model/STTODE.py:463-486: past_traj [B,N,Tp,2],
 * future_traj [B,N,Tf,2]): a [na] and b [nb] floats (HOST, pageable; b may be NULL with nb = 0) -> dev [na4 + nb] (DEVICE; a at 0, b at
 * na4 = na rounded up to a multiple of 4, so both start on 16-byte boundaries) with one
 * asynchronous copy on `stream` (a pageable `.to(device)` waits for everything queued on the stream: in train.py:61-67 the previous step). */
int sttode_stage_rows(const float* a, long na, const float* b, long nb, float* dev, void* stream);
/* The pipeline stream the next sttode_inference_*_async call of n agents will run on (*stream; NULL when the call will not take the
 * one-stream fused form).  Inputs prepared on that stream, and the call issued from it, need no cross-stream event. */
int sttode_async_next_stream(SttodeModel* m, int n, void** stream);
/* Best-of-K ADE / FDE of an asynchronous call's predictions (utils/metrics.py:7-26, as sttode_best_of_k) enqueued on the pipeline stream
 * the call of `slot` runs on: the metrics start the moment the call's launch drains, in stream order.  Re-records the slot's completion
 * event behind them (sttode_wait(slot) then covers the metrics).  gt must have been written before the sttode_inference_*_async call
 * (its stream waits for the caller's stream at that point). */
int sttode_async_best_of_k(SttodeModel* m, int slot, const float* pred, const float* gt, int n, int K, int Tf, float scale, float* ade,
                           float* fde);
/* Serial scene calls (sttode_inference_scenes) below the chain threshold -- the reference's evaluation loop hands over ONE scene per call
 * (test.py:171-188) -- run as ONE launch whose workgroups take the roles front-end + per-agent stage / block-0 decoder_y / block-0
 * decoder_x -> block-1 GRU -> block-1 decoder_y and hand tables over through flags (csrc/scene_lat.hip), when the call has at most
 * `max_tiles` 16-trajectory tiles: -1 = default (128), 0 = never (six launches, as round 2).  Bitwise the
 * same predictions either way.  Replaces: model/STTODE.py:397-461 + :553-627 for one scene. */
int sttode_set_scene_launch(SttodeModel* m, int max_tiles);
/* integrator of the tensor-ODE encoder inside the native pipeline: method / steps as in sttode_post_attn_ode (default 0, 1 = reference).
 * Attention length 1 (scene batches): every stage inside the fused encoder kernel.  Attention groups > 1 (sttode_inference_nba): every
 * stage is a pass over the group -- in-projection of the state, sttode_mhgsa_attn, sttode_post_attn_rhs, axpy combinations -- enqueued
 * natively by the same call (odeint over TransformerEncoder_ode, ode_demo.py:186-190; parity unpinned: the reference only takes one Euler step). */
int sttode_set_ode(SttodeModel* m, int method, int steps);
/* every = 0: off; n > 0: bracket the stages of every n-th forward call with hipEvents recorded on the launch streams (the
 * per-trajectory stages are bracketed on every call while n > 0) */
int sttode_timing_enable(SttodeModel* m, int every);
/* total_ms: sum of the launches' durations; busy_ms (optional): length of the union of their [start, end] intervals -- launches of
 * consecutive pipelined calls overlap, so a stage's rate is work / busy time, not work / mean launch duration. */
int sttode_timing_read(SttodeModel* m, double* total_ms /*[STT_STAGE_COUNT]*/, int* launches /*[STT_STAGE_COUNT]*/,
                       double* busy_ms /*[STT_STAGE_COUNT] or NULL*/);

/* set_data (batched over scenes) + inference (model/STTODE.py:397-461,574-623; caller loop test.py:171-184).
 * past [n,Tp,2] world coords, scene_ptr [S+1], z [n*K,32] -> pred [n,K,Tf,2] world coords. */
int sttode_inference_scenes(SttodeModel* m, const float* past, const int* scene_ptr, int n, int S, const float* z,
                            float* workspace, float* pred, void* stream);
/* set_data_nba + inference, NBA branch (model/STTODE.py:463-486,578-583; caller test.py:520-524):
 * past [B*N,Tp,2]; attention length = B over the N agent slots. */
int sttode_inference_nba(SttodeModel* m, const float* past, int B, int N, const float* z, float* workspace, float* pred,
                         void* stream);
/* G forward-call batches of the NBA branch in ONE call (what G sttode_inference_nba calls compute; the reference's evaluation loop makes one
 * model call per DataLoader batch, test.py:520-524): past [G][B][N][Tp][2], z [G B N K][32] -> pred [G B N][K][Tf][2].  The attention
 * (Hyp_mhsa over the batch dimension, hyptransformerlib.py:261-265) runs within each batch of B scenes -- one launch with a group dimension
 * -- and everything per agent / per trajectory over all G B N agents: a test set of 128-scene batches fills the chip. */
int sttode_inference_nba_groups(SttodeModel* m, const float* past, int G, int B, int N, const float* z, float* workspace, float* pred,
                                void* stream);

/* Pipelined forms (STTODENet.inference as a stream of calls, model/STTODE.py:574-623; caller loop test.py:171-184): consecutive calls run
 * on the pipeline's internal streams so that the grid tail of one call's big launch is filled by the next call's.
 *   LAGGED form (round 4; default for every call whose per-trajectory stage takes the chain, reference integrator): calls rotate over
 *   `streams` pipeline streams (sttode_set_lagged; default 3); the ONE launch a call enqueues carries ITS per-agent stage in throughput form
 *   (128 agents per workgroup, csrc/role32.hpp) followed by the trajectory groups of the call made `streams` calls earlier on the same
 *   stream -- whose per-agent tables the previous launch of that stream produced.  Nothing inside a launch depends on anything else in it
 *   (no flags, no spinning).  A call's predictions are therefore produced by the launch of a LATER call -- or by sttode_wait(slot) /
 *   sttode_async_best_of_k(slot), which enqueue the outstanding groups of that slot as a launch of their own if no later call has done so.
 *   Slots: up to 8 (slot in [0, 8)); a loop that keeps 2 x streams calls in flight never waits on another stream.  Agrees with the serial
 *   forms to fp32 rounding (different MFMA tiling and host-folded embedding in the per-agent stage), not bitwise.
 *   sttode_set_lagged(m, 0): the round-3 forms (fused launches of one call each on three streams / separate per-agent launches), bitwise
 *   the serial forms.  Calls below the chain threshold or with a non-default integrator always take those forms.
 * workspace, pred and z of a slot must stay untouched until sttode_wait(slot) has been enqueued on the consuming stream. */
int sttode_set_lagged(SttodeModel* m, int streams /* 0 = off, 2 or 3 (default, or env STTODE_LAGGED) */);
/* Per-call options of the asynchronous entry points (NULL = none).  Everything a call needs travels WITH the call: a request the call's
 * form cannot honour makes the call fail before anything is enqueued or any state of the model changes (ABI <= 6 armed the model with
 * sttode_async_device_latents / sttode_async_fused_metrics before the call; a failed check in between left the request armed).
 *   device_latents != 0 (lagged form only; replaces the torch.randn_like of Normal.rsample, model/STTODE.py:89-93,609-616, for that call): the
 *     call treats its `z` argument as an OUTPUT buffer [n K][32] which its own per-agent roles fill with N(0, I) samples (Philox4x32-10, 64-bit
 *     key zkey, counter = the float4's index; two Box-Muller pairs per block) before its trajectory groups read it.
 *   metrics_gt != NULL (lagged form only; replaces a sttode_best_of_k launch per call): the call's trajectory groups also compute its
 *     min-over-K ADE / FDE (compute_ADE / compute_FDE, utils/metrics.py:7-26; the values of sttode_best_of_k on the same predictions, bit for
 *     bit) against metrics_gt [n][Tf][2], scaled by metrics_scale, into ade / fde [n]; valid once sttode_wait(slot) has passed.
 *   nba_groups > 1 (sttode_inference_nba_async only): the call carries that many forward-call batches [G][B][N][Tp][2]; the attention runs
 *     within each batch of B scenes (sttode_inference_nba_groups).
 *   sampler != NULL (lagged form only; ABI 8): the call's latents come from the stage-2 sampler's Q-net (SttodeSamplerPlan; sampler.py:39-54,
 *     test_sampler.py:136) instead of the caller: `z` is an OUTPUT buffer [n K][32], filled on the call's pipeline stream from the past
 *     features its own per-agent roles wrote, before its trajectory groups read it.  Refused (before anything is enqueued) together with
 *     device_latents, on a call that is not in the lagged form, and for a plan whose widths the Q-net kernel cannot stream.
 * sttode_async_is_lagged(m, n) tells beforehand whether a call of n agents will take the lagged form. */
/* Stage-2 latent sampler (sampler.py:32-54) as a weight stream: the Q-net  h = linear(pf) 128 -> 64,  two tanh layers 64 -> h1 -> h2
 * (utils/mlp.py:5-29, qnet_mlp; default 512, 256),  per sample k: b_k = q_b h (and A_k = q_A h when eps is given),  z_k = A_k eps + b_k
 * (sampler.py:41-51; eps_mode 0: z = b (mean), 1: eps [nz] shared by every agent, 2: eps [n][nz] per agent).  pool / prog: PK32 tiles and
 * the chunk program of the eps mode (sttode_amd/packing.py sampler_stream: mean mode skips the q_A tiles); biases:
 * [linear 64 | layer 1 h1 | layer 2 h2 | q_b K nz | q_A K nz].  Streamable: nz == 32, h1 and h2 multiples of 32, h2 <= 256, prog_len <= 4096. */
typedef struct SttodeSamplerPlan {
    const float* pool;
    const int* prog;
    int prog_len;
    const float* biases;
    int K;
    int nz;
    int h1;
    int h2;
    int eps_mode;
    const float* eps;
} SttodeSamplerPlan;
typedef struct SttodeAsyncOpts {
    int device_latents;
    unsigned long long zkey;
    const float* metrics_gt;
    float* ade;
    float* fde;
    float metrics_scale;
    int nba_groups;
    const SttodeSamplerPlan* sampler;
} SttodeAsyncOpts;
/* The sampler's Q-net as one launch (sampler.py:39-54; the latents test_sampler.py:136 decodes): past features pf [n][128] -> z [n K][nz],
 * row agent K + k; 128 agents per workgroup, weights streamed through LDS.  Serves every call that has no lagged per-agent stage. */
int sttode_sampler_qnet(const SttodeSamplerPlan* plan, const float* pf, int n, float* z, void* stream);
/* Measurement aid: the shader clock at this moment.  out[0] = shader cycles, out[1] = ticks of the constant 100 MHz clock over ~20 us on
 * one lane (device memory, two int64): GHz = out[0] / (10 out[1]). */
int sttode_clock_probe(long long* out, void* stream);
/* Device -> pinned host copy of `bytes` (multiple of 16; both pointers 16-byte aligned; dst: device-accessible host memory) by `wgs`
 * persistent workgroups (<= 0: 8) on `stream`: a copy that leaves the chip's workgroup slots to the kernels running beside it. */
int sttode_copy_to_host(void* dst, const void* src, long bytes, int wgs, void* stream);
/* Enqueue the outstanding trajectory-group launch of the call in `slot` now (no-op when a later call has carried it already). */
int sttode_async_enqueue(SttodeModel* m, int slot);
/* Enqueue every outstanding trajectory-group launch of the lagged form (before buffers of pending calls are released or reused). */
int sttode_async_flush(SttodeModel* m);
int sttode_inference_scenes_async(SttodeModel* m, const float* past, const int* scene_ptr, int n, int S, const float* z,
                                  float* workspace, float* pred, int slot, const SttodeAsyncOpts* opts, void* stream);
int sttode_inference_nba_async(SttodeModel* m, const float* past, int B, int N, const float* z, float* workspace, float* pred,
                               int slot, const SttodeAsyncOpts* opts, void* stream);
/* sttode_horizon_metrics of an asynchronous call's predictions on the pipeline stream the call of `slot` runs on (as sttode_async_best_of_k:
 * starts the moment the call's groups drain; the slot's completion event is re-recorded behind it). */
int sttode_async_horizon_metrics(SttodeModel* m, int slot, const float* pred, const float* gt, int n, int K, int Tf, float scale, float* out);
/* sttode_best_of_k_select of an asynchronous call's predictions (utils/metrics.py:7-48, test.py:193-205) on the pipeline stream the call of
 * `slot` runs on, as sttode_async_best_of_k: the slot's outstanding trajectory groups are enqueued first, the selection follows them in stream
 * order, and the slot's completion event is re-recorded behind it.  gt and seg_ptr must have been written before the call. */
int sttode_async_best_of_k_select(SttodeModel* m, int slot, const float* pred, const float* gt, int n, int K, int Tf, float scale,
                                  float miss_threshold, const int* seg_ptr, int S, float* ade, float* fde, int* best_ade_idx, int* best_fde_idx,
                                  unsigned char* miss, float* best, float* seg_ade, float* seg_fde, int* seg_miss);
/* sttode_joint_select / sttode_kde_nll of an asynchronous call's predictions on the pipeline stream the call of `slot` runs on, as
 * sttode_async_best_of_k_select: the slot's outstanding trajectory groups first, the pass behind them in stream order, the slot's completion
 * event re-recorded behind it.  gt and seg_ptr must have been written before the call; arguments are checked before anything is enqueued. */
int sttode_async_joint_select(SttodeModel* m, int slot, const float* pred, const float* gt, int n, int K, int Tf, float scale,
                              const int* seg_ptr, int S, float radius, float* seg_jade, float* seg_jfde, int* seg_jade_idx, int* seg_jfde_idx,
                              int* seg_col, int* seg_gt_col);
int sttode_async_kde_nll(SttodeModel* m, int slot, const float* pred, const float* gt, int n, int K, int Tf, float scale, double* nll);
/* sttode_sample_spread of an asynchronous call's predictions, on the call's pipeline stream behind its outstanding groups, the slot's
 * completion event re-recorded behind it (as sttode_async_kde_nll). */
int sttode_async_sample_spread(SttodeModel* m, int slot, const float* pred, const float* gt, int n, int K, int Tf, float scale,
                               double div_scale, double* apd, double* fpd, double* pade, double* dlow, double* es_ade, double* es_fde,
                               float* ade_at_k, float* fde_at_k);
int sttode_wait(SttodeModel* m, int slot, void* stream);
/* Zero-copy futures (lagged form): the trajectory groups of a lagged call only WRITE `pred` (block 0's y_hat0 waits in the workspace), so
 * `pred` may be pinned host memory addressed by its host pointer: the futures reach the host with the launch itself, no D2H copy
 * (test.py:186-188 moves every prediction to NumPy).  sttode_async_is_lagged: 1 if the next async call of n agents takes that form (a
 * query, not a status); sttode_wait_host: the HOST waits for the call of `slot` (its outstanding groups are enqueued first). */
int sttode_async_is_lagged(SttodeModel* m, int n);
int sttode_wait_host(SttodeModel* m, int slot);
/* Health of the in-launch hand-off (round-3 fused launches and the one-launch scene form: a group whose producer never signalled gives up
 * after ~1 s, poisons its predictions with NaN and sets the launch's time-out word -- in the workspace AND in the model's word in pinned
 * host memory).
 * sttode_timeout_word: *word = address of the model's host-visible time-out word (valid for the model's life): non-zero once ANY launch of
 * this model gave up since the last sttode_timeout_clear.  Reading it costs a host load -- no stream operation, no synchronisation -- so a
 * caller checks it at its next call and before handing results out (STTODENet.inference() / wait() do, and raise).  The word is set when
 * the group gives up, i.e. it is seen by whoever looks after the launch has finished.
 * sttode_check: reads the time-out word of the LAST launch that used `workspace` (laid out for n agents / S scenes) after synchronising
 * `stream`: returns 0 if it is clear, 3 (and sttode_last_error) if a group gave up or the workspace was never initialised -- the caller's
 * predictions of that call are not valid.  Lagged launches have no hand-off and always pass. */
int sttode_timeout_word(SttodeModel* m, const unsigned** word);
int sttode_timeout_clear(SttodeModel* m);
int sttode_check(SttodeModel* m, const float* workspace, int n, int S, void* stream);

#ifdef __cplusplus
}
#endif
#endif
