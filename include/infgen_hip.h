/*
 * infgen_hip.h — C ABI of libinfgen_hip.so: the MI355X (gfx950) implementation of InfGen's
 * closed-loop rollout hot path.
 *
 * The reference (OrangeSodahub/InfGen) is pure Python and has no FFI for this path; its native
 * arithmetic lives in third-party wheels.  Each entry point below replaces one group of those
 * calls (file:line are relative to the reference repository):
 *
 *   infgen_linear            torch.nn.Linear / LayerNorm / ReLU chains: MLPEmbedding, MLPLayer
 *                            (infgen/modules/layers.py:163-215)
 *   infgen_fourier_embed     FourierEmbedding.forward (infgen/modules/layers.py:142-160)
 *   infgen_attn_pre          AttentionLayer: prenorm + to_q/to_k/to_v (+ absorbed to_k_r)
 *                            (infgen/modules/layers.py:65-73,106-108)
 *   infgen_edge_attn         MessagePassing.propagate + torch_geometric.utils.softmax
 *                            (infgen/modules/layers.py:78-92,109)
 *   infgen_attn_post         AttentionLayer.update / to_out / post-norm / FFN
 *                            (infgen/modules/layers.py:74-75,94-99,110-112)
 *   infgen_heads             token_predict_head / state_predict_head + greedy arg-max
 *                            (infgen/modules/agent_decoder.py:2161-2167)
 *   infgen_heads_logprob     the same + the log-probability of the chosen token (pred_prob, agent_decoder.py:1689 / :2205)
 *   infgen_map_token_head    the map encoder's token_predict_head + top-10 (infgen/modules/map_decoder.py:119-121)
 *   infgen_map_graph         torch_cluster.radius_graph over map tokens + relative features
 *                            (infgen/modules/map_decoder.py:91-114)
 *   infgen_build_edges       _build_temporal_edge / _build_interaction_edge / _build_map2agent_edge
 *                            incl. torch_cluster.radius(max_num_neighbors=5)
 *                            (infgen/modules/agent_decoder.py:540-758)
 *   infgen_integrate         token -> contour -> pose, Attr_Tokenizer.encode_pos, invalid handling
 *                            (infgen/modules/agent_decoder.py:2168-2239, attr_tokenizer.py:77-89)
 *   infgen_raw_feature       _build_vector_a / x_a_emb / fusion_emb for one column
 *                            (infgen/modules/agent_decoder.py:426-509,2265-2287)
 *   infgen_decode_layers     the 6 x (temporal, map->agent, agent<->agent) stack on one column
 *                            (infgen/modules/agent_decoder.py:2123-2158)
 *   infgen_decode_step       one iteration of the rollout loop (infgen/modules/agent_decoder.py:1740-2301,
 *                            insertion disabled)
 *   infgen_point_edges, infgen_occupancy, infgen_insert_decide, infgen_insert_finalize, infgen_raw_feature_rows
 *                            the insertion sub-loop (infgen/modules/agent_decoder.py:1773-2105)
 *   infgen_command_rows      no counterpart: a controller's per-step commands (token ids or target poses) for the replayed rows
 *   infgen_branch_scenes, infgen_resample_parents   no counterpart: a copy of a scene continues as a clone of another copy
 *   infgen_snapshot_scenes, infgen_restore_scenes, infgen_snapshot_bytes   no counterpart: a slot's decode state saved and put back
 *
 * and, around the path:
 *
 *   infgen_tokenize_agent, infgen_match_agent_tokens   TokenProcessor (infgen/datasets/preprocess.py:335-653)
 *   infgen_match_map_tokens, infgen_fetch_enterings    InfGen.match_token_map / _fetch_enterings
 *                                                      (infgen/model/infgen.py:918-984, 1008-1128)
 *   infgen_distance_to_nearest_object, infgen_time_to_collision, infgen_kinematic_features,
 *   infgen_distance_to_road_edge, infgen_placement_features   infgen/metrics/{interact,trajectory,map,placement}_features.py
 *   infgen_window_log_likelihood                       the scoring of LongMetric (infgen/metrics/compute_metrics.py:845-878)
 *   infgen_bundle_scores                               the same for all rollouts of all scenarios of a batch (:891-1103)
 *   infgen_state_accuracy, infgen_grid_overlap, infgen_traj_error, infgen_token_cls, infgen_average_meter,
 *   infgen_masked_cross_entropy                        the validation step's bookkeeping (infgen/utils/metrics.py) and open-loop loss
 *   infgen_select_modes, infgen_multi_traj_error       K modes per agent from the copies' rollouts (batch_nms / new_batch_nms,
 *                                                      infgen/utils/metrics.py:143-256) and minMultiADE / minMultiFDE (:339-427)
 *
 * Conventions: every pointer is a DEVICE pointer (fp32 / int32 / uint8) borrowed for the duration
 * of the call; outputs are pre-allocated by the caller; `stream` is a hipStream_t; nothing
 * synchronises with the host; functions return 0 on success or a negative code and leave a message
 * retrievable with infgen_last_error() (thread-local).
 * Re-entrancy: every switch that changes what a launch computes (kernel family, arithmetic, rhat row format, overlap, padded-row lists)
 * is a field of InfgenOptions.  A rollout context carries its own block (InfgenRollout.opts, use = 1) and a thread may install one for
 * the operator-level entries (infgen_thread_options): contexts with different arithmetic coexist in one process.  The infgen_set_*
 * functions only edit the process-wide DEFAULT block that contexts / threads without their own inherit.  Environment variables
 * (INFGEN_*) are tuning thresholds and diagnostics of the launch shapes (which kernel variant from how many rows); each is read once
 * per process and none changes the arithmetic.
 * Style: infgen_amd/_lib.py reads its ctypes binding from this file and refuses what is not in use here - `#define NAME integer`, anonymous
 * enums, `typedef struct X {..} X;` of scalars, pointers (one name each), fixed arrays, earlier structs; int / const char* functions, named parameters.
 */
#ifndef INFGEN_HIP_H_
#define INFGEN_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INFGEN_MAX_LAYERS 8

/* offsets / sizes (floats) of the packed weight layouts, see infgen_amd/csrc/layout.h */
enum {
  INFGEN_Q_ATTN_PACK_SIZE = 0,
  INFGEN_Q_FOURIER_PACK_SIZE_N2 = 1,
  INFGEN_Q_FOURIER_PACK_SIZE_N3 = 2,
  INFGEN_Q_FOURIER_PACK_SIZE_N4 = 3,
  INFGEN_Q_TILE_ROWS = 4,
  INFGEN_Q_EDGE_ATTN_CAP = 5,
  INFGEN_Q_MAX_AGENTS = 6,
  INFGEN_Q_ABI_VERSION = 7,
  INFGEN_Q_SIZEOF_ROLLOUT = 8,
  INFGEN_Q_ATTN_SPLIT_ROWS = 9,   /* attn_mode 2 takes the split kernels (and the fused token log-probability) beyond this many rows */
  INFGEN_Q_HEADS_SAMPLE_K = 10,   /* the widest top-k beam the split heads kernel samples itself (infgen_heads_sample_fused) */
};
int infgen_layout_query(int what);
/* offset (floats) of a named field inside the AttentionLayer / Fourier pack; -1 if unknown */
int infgen_attn_pack_offset(const char* field);
int infgen_fourier_pack_offset(const char* field, int n_dims, int dim);
const char* infgen_last_error(void);

typedef struct InfgenEdgeBuf {
  int* off;      /* [rows] */
  int* cnt;      /* [rows] */
  int* src;      /* [cap] */
  float* raw;    /* [cap][4] */
  float* rhat;   /* [cap][128] fp32 as written by infgen_fourier_embed.  The three sets of an InfgenRollout (et / em / ea) are scratch of
                  * infgen_decode_layers: between its Fourier and edge launches it may keep the rows in a packed 24-bit form (384 B
                  * per row in the same buffer) - do not read them back */
  int* total;    /* [1] */
  int cap;
  int _pad;
} InfgenEdgeBuf;

/* kernel-selection switches and the padded-row bookkeeping of one rollout context (see InfgenRollout.opts) */
typedef struct InfgenOptions {
  int use;              /* 0: the process-wide defaults of the infgen_set_* functions apply (single-context callers) */
  int attn_mode;        /* infgen_set_attn_mode */
  int gemm_terms;       /* infgen_set_gemm_terms */
  int fourier_mode;     /* infgen_set_fourier_mode */
  int edge_fuse;        /* infgen_set_edge_fuse */
  int edge_loop;        /* infgen_set_edge_loop */
  int overlap;          /* infgen_set_overlap (the side stream itself is shared: keep 0 when contexts run concurrently) */
  int row_group_margin; /* rows a decode step may append (infgen_set_row_limits) */
  int layers_p;         /* infgen_set_layers_p: 1 = small launches run a decode step's sublayers in one launch (k_layers_p) */
  int rhat_format;      /* infgen_set_rhat_format: 0 (default) fp32 rows of the normalised relative-position embedding between the
                         * Fourier and the edge kernels, 1 packed 24-bit rows (384 B, 2^-17 relative: a reduced-precision mode) */
  int edge_kernel;      /* infgen_set_edge_kernel: lane layout of the fused edge kernel's loop - 0: lane = two columns of every row
                         * (k_edge_fused), 1 (default): lane = (head, 16-column slice) with the rhat rows staged through LDS
                         * (k_edge_fused3) for launches beyond 4 k rows, 2: the same at every size.  Same results up to fp32
                         * summation order; packed 24-bit rhat rows (rhat_format 1) always take k_edge_fused. */
  int _pad0;
  const int* row_groups; const int* n_row_groups;   /* optional list of the 16-row groups that hold agents (infgen_set_row_groups) */
} InfgenOptions;

/* temperature and nucleus (top-p) truncation of the top-k samplers (infgen_sample_topk_ex, infgen_heads_sample_ex,
 * infgen_insert_decide_topk_ex; InfgenRollout.sample_* / InfgenInsertion.insert_*).  With v[0..k-1] a row's k best logits in the
 * samplers' total order (value descending, column ascending), it = 1 / T in fp32 and u01 the caller's uniform:
 *   1. p[j] = expf((v[j] - v[0]) * it), cdf[j] the running sum in j order, S_k = cdf[k-1]
 *   2. the nucleus size m: the smallest m with cdf[m-1] >= top_p * S_k - the nucleus of the re-normalised top-k distribution (top-k
 *      first, then top-p); always m >= 1; top_p >= 1: m = k, no comparison made
 *   3. sum = cdf[m-1], u = u01 * sum, pick = the first j < m with u < cdf[j], else m - 1
 *   4. sample_logprob = (v[pick] - v[0]) * it - logf(sum); token_logprob stays the model's own full softmax at temperature 1
 *   5. a row with T == 0 is greedy: pick = 0, sample_logprob = 0 (its uniform is still read)
 * temperature: finite, >= 0 and no denormal (1 / T must stay finite); top_p in (0, 1]; 0 means "unset" and equals 1 for both (a zero-filled struct is the plain top-k sampler,
 * bit for bit); anything else is refused.  temperature_row (optional, [rows], entries >= 0) wins over the scalar, and there 0 means
 * greedy (as does any entry below the smallest normal float); it is device memory and not checked by the library.  k <= 1: the arg-max, the parameters are ignored. */
typedef struct InfgenSampling {
  float temperature; float top_p;
  const float* temperature_row;
} InfgenSampling;

/* constrained decoding: per-row allowed-token sets of the motion-token heads and samplers.  A TOKEN MASK is five values, passed as
 * the parameters (mask_bits, mask_n_sets, mask_row, mask_type, type) of infgen_heads_sample_mask / infgen_sample_topk_mask, or
 * registered once (infgen_token_mask_create) and named by InfgenRollout.token_mask:
 *   - mask_bits is a mask table: mask_n_sets bit sets of token_size bits each, every set token_size / 32 little-endian uint32 words;
 *     bit c of a set (word c / 32, bit c % 32) set means token c is allowed.  Every set allows at least one token (a set without one
 *     breaks the contract: its rows emit token 0).  Device memory, 16-byte aligned.
 *   - the set of a row: mask_row[row] (optional, device int32 [rows]) where it is >= 0; otherwise mask_type[type[row]] (mask_type:
 *     three HOST ints, NULL = all -1; type: device int32 [rows] with 0 vehicle, 1 pedestrian, 2 cyclist; any other type value, and
 *     -1 in mask_type, mean unconstrained).  A set index >= mask_n_sets reads as unconstrained: nothing outside the table is ever read.
 *   - a banned column's logit counts as -inf for the arg-max, the running top-k and the draw; equal logits still go to the lower
 *     allowed column.  With a allowed tokens and beam k the draw is InfgenSampling's over min(k, a) entries, so no banned token is
 *     emitted for any uniform in [0, 1) - 1 - 2^-24 included, where step 3's "else m - 1" would otherwise name a slot of probability 0.
 *   - stored logits stay the model's raw logits, and token_logprob keeps its meaning: the model's full, unmasked softmax of the
 *     emitted token.  sample_logprob is the log-probability under the sampler's actual distribution (mask, then top-k, temperature,
 *     top-p); a greedy row gives 0.
 *   - the state head, the insertion cell draw and replayed, commanded or teacher-forced rows are left alone.
 *   - mask_bits == NULL, mask_n_sets == 0, or mask_row == NULL with every mask_type -1: today's kernels, today's bits.
 * Refused: mask_n_sets < 0, a table without `type` while any mask_type is >= 0, a token_size that is no multiple of 32, a misaligned
 * table.  (Parameters and a handle, not a struct and new InfgenRollout members: tests pin the header's set of structs and
 * sizeof(InfgenRollout).) */

typedef struct InfgenRollout {
  /* sizes / hyper-parameters */
  int S, A_cap, T, M_cap, W, ring, R, token_size, grid_size, num_layers;
  int force_valid;      /* disable_insertion: predicted states are overridden with 'valid' */
  int store_logits;     /* 1: logits[t] is written every step */
  float r_map, r_agent; /* pl2a_radius, a2a_radius */
  /* scene state, column-major per scene: [S][T][A_cap] */
  const int* n_agents; const int* n_map; const int* av_index;
  float* pos; float* head; int* state; int* token; int* grid;
  uint8_t* tmask; uint8_t* imask; uint8_t* catflag;
  const int* type; int* bos;
  const float* map_pos; const float* map_orient;
  /* packed weights */
  const float* attn_t[INFGEN_MAX_LAYERS]; const float* attn_m[INFGEN_MAX_LAYERS]; const float* attn_a[INFGEN_MAX_LAYERS];
  const float* four_t; const float* four_m; const float* four_a; const float* four_xa;
  const float* fusion_pack;    /* MLPEmbedding(512; 384 with no_grid_token): P(K0,128) b ln | P(128,128) b ln | P(128,128) b */
  const float* tok_head_pack; const float* st_head_pack;
  const float* tok_tab; const float* grid_tab; const float* state_emb;
  const float* cat_agent; const float* cat_seed; const float* vocab; const float* grid_xy;
  /* caches */
  float* ringK[INFGEN_MAX_LAYERS]; float* ringV[INFGEN_MAX_LAYERS];         /* [ring][rows][128] */
  const float* mapK[INFGEN_MAX_LAYERS]; const float* mapV[INFGEN_MAX_LAYERS]; /* [S*M_cap][128] */
  /* scratch */
  float* X; float* Q; float* U; float* Ka; float* Va; float* AGG; float* Z; float* SIG;
  InfgenEdgeBuf et, em, ea;
  float* raw2; float* cat; float* fus_in; float* tmp1; float* tmp2;
  int* next_token; int* next_state;
  float* logits;               /* optional [steps][rows][token_size] */
  const int* teacher_token; const int* teacher_state;   /* optional [S][T][A_cap] */
  /* outputs */
  float* pred_traj; float* pred_head; float* pred_state;   /* [S][A_cap][R](x2) */
  /* scenario insertion (optional, NULL when unused): rows >= first_new[s] inserted in the current step use
   * hv_ovr[s] as their head vector during the motion stage (agent_decoder.py:2083) */
  const int* first_new; const float* hv_ovr;
  /* reproducible top-k sampling (optional): sample_k > 1 -> every step draws the motion token by inverse CDF over
   * the sample_k most probable tokens with the uniforms sample_u[t][row]; needs logits_scratch [rows][token_size] unless every
   * step samples inside the heads kernel (infgen_heads_sample_fused(attn_mode, S * A_cap, sample_k)) */
  int sample_k;
  /* constrained decoding: 0 (none) or a handle of infgen_token_mask_create - infgen_decode_step applies that mask to the motion token
   * of every row, greedy or sampled (rows scenario insertion appends have mask_row -1 and take their type's set), and
   * infgen_rollout_run takes the per-step path while a mask is active.  Takes the place of a padding word: the struct did not grow. */
  int token_mask;
  const float* sample_u; float* logits_scratch;
  /* per-context options (re-entrancy): with opts.use != 0 the rollout-level entries (infgen_decode_layers / _step /
   * infgen_rollout_run, infgen_raw_feature*, infgen_build_edges) take every switch from here and never read the process-wide
   * defaults of the infgen_set_* functions - two contexts of one process may differ and run from different host threads */
  InfgenOptions opts;
  /* optional [S][T][A_cap]: grid cell of the teacher-forced state per (column, row); entries < -1 mean "none" (the cell is
   * computed).  Long teacher-forced comparisons use it where a pose sits on a cell border (arg-min of encode_pos flips with
   * the last bits of the pose) */
  const int* teacher_grid;
  /* optional [32][128], written by infgen_fourier_last_dim_table(four_t, 4, ..) under the arithmetic (infgen_set_gemm_terms /
   * opts.gemm_terms) the context runs with: the temporal edges' time-gap input takes the values -1 .. -16 only, so its branch
   * of r_t_emb (layers.py:150-153, mlps[3]) is looked up instead of evaluated per edge.  NULL: evaluated per edge. */
  const float* four_t_dt;
  /* optional [S][T][A_cap][2] / [S][T][A_cap]: pose of the teacher-forced state per (column, row).  When given, the pose a decode step
   * stores for its new column is the teacher's (rows the teacher marks invalid excepted); the step's OWN result still goes to
   * pred_traj / pred_head.  Every step then starts from the same geometry as the reference run, so a long comparison has no
   * accumulated pose drift and no radius / first-K decision can flip: logits are comparable row by row with a maximum, and the
   * one-step pose update is checked separately (tests/test_baseline_shapes_gpu.py) */
  const float* teacher_pos; const float* teacher_head;
  /* optional [S][A_cap] (log replay): with it, teacher_token / teacher_state / teacher_grid / teacher_pos / teacher_head apply only
   * to the rows flagged 1 - they follow the plan (the logged future or a planner's) - and every other row is generated exactly
   * as without a teacher.  NULL: the teacher arrays, when given, apply to every row.  Needs teacher_token and teacher_state
   * (infgen_rollout_validate).  Rows scenario insertion appends are never flagged. */
  const unsigned char* replay_row;
  /* optional [S]: the map-side scene of agent-side scene s (NULL: s itself).  Several scenes may share ONE set of map tokens - n_map,
   * map_pos / map_orient, the rows [slot * M_cap, (slot + 1) * M_cap) of mapK / mapV (and of InfgenInsertion.mapK / mapV) are then
   * indexed by slot = map_scene[s]: the n rollouts of one scene (reference infgen/model/infgen.py:704-706, inference_no_map
   * infgen_decoder.py:132-134) encode their map once and keep one copy of its K / V rows */
  const int* map_scene;
  /* optional [num_layers][S * A_cap][128] (test hook): infgen_decode_layers copies the residual stream X there after every
   * (temporal, map -> agent, agent <-> agent) triple - the reference's feat_a after a2a_attn_layers[i] for the current column
   * (infgen/modules/agent_decoder.py:2133-2158).  A context with tap_x runs the per-sublayer launches (k_layers_p keeps the
   * stream in registers across the triples) */
  float* tap_x;
  /* temperature / nucleus mass of the motion-token draw (InfgenSampling: 0 = unset = 1) and an optional per-row temperature
   * [S * A_cap] that wins over the scalar (0: that row decodes greedily, sample_logprob 0) - a batch of copies is a temperature sweep.
   * Read by sampling steps only (sample_k > 1 with sample_u); token_logprob is not tempered.  Placed in front of sample_logprob,
   * token_logprob and the two ablation switches, whose places at the struct's end older tests pin; INFGEN_Q_SIZEOF_ROLLOUT covers the growth, INFGEN_Q_ABI_VERSION keeps answering 1.
   * infgen_heads_sample_fused and the need for logits_scratch do not depend on them. */
  float sample_temperature; float sample_top_p;
  const float* sample_temp_row;
  /* optional [steps][S * A_cap]: infgen_decode_step writes step t's slice with the log-probability of the sampled motion token under
   * the sampler's OWN distribution (the softmax re-normalised over the sample_k best logits) - laid out and overridden like
   * token_logprob, independent of it.  Written by sampling steps only (sample_k > 1 with sample_u): a greedy step leaves the slice
   * as it is - the sampler is a point mass there, so a zeroed buffer already holds the answer.  It sits in front of token_logprob and the two
   * ablation switches, whose places at the struct's end older tests pin; INFGEN_Q_SIZEOF_ROLLOUT covers the new size. */
  float* sample_logprob;
  /* optional [steps][S * A_cap]: infgen_decode_step writes step t's slice with the FULL-softmax log-probability of the motion token
   * every row emitted (log_softmax(logits)[next_token], after sampling where sample_k > 1) - every row of the layout, padding
   * included; rows whose token is then overridden (teacher / replay, invalid state) keep the value of the head's own token.
   * Contexts on the split path (attn_mode 1, or 2 beyond 10240 rows) that decode greedily or sample inside the heads kernel
   * (infgen_heads_sample_fused) compute it there and need no logits in memory; every other context needs store_logits or
   * logits_scratch (refused otherwise).  infgen_rollout_run does
   * not fold the step tail while it is set.  Added in front of the two ablation switches, which stay the
   * struct's last members (tests/test_ablation_cpu.py pins that): their offsets moved by 8 bytes, INFGEN_Q_SIZEOF_ROLLOUT covers
   * the new size, and INFGEN_Q_ABI_VERSION keeps answering 1 (a test pins that too; the Python binding checks the size, not the
   * version, at load - rebuild both sides together). */
  float* token_logprob;
  /* the reference's token ablations (agent_decoder.py use_grid_token / use_state_token; 0 = the full-token model).
   * no_grid_token: the fusion embedding takes [token | x_a | state] (fusion_pack packed with K0 = 384, fus_in keeps its 512
   * stride) and no grid_tab row is gathered.  no_state_token: after the ego override a predicted 'exit' becomes 'valid'. */
  int no_grid_token; int no_state_token;
} InfgenRollout;

int infgen_linear(const float* X, int ldx, const int* gather, int rows, int K,
                  const float* Wp, int Np, const float* bias, int N,
                  const float* pre_g, const float* pre_b, const float* post_g, const float* post_b, int relu,
                  float* Y, int ldy, void* stream);

/* n (<= 6) independent infgen_linear calls in one launch (the heads of the insertion sub-loop); fields as infgen_linear's
 * arguments */
typedef struct InfgenLinearDesc {
  const float* X; int ldx; const int* gather; int rows; int K;
  const float* Wp; int Np; const float* bias; int N;
  const float* pre_g; const float* pre_b; const float* post_g; const float* post_b; int relu;
  float* Y; int ldy;
} InfgenLinearDesc;
int infgen_linear_multi(const InfgenLinearDesc* desc, int n, void* stream);
/* MLPEmbedding.forward (infgen/modules/layers.py:163-192) for inputs of K0 = 128 j <= 512 columns: Linear LN ReLU Linear LN ReLU
 * Linear, pack = infgen_amd.packing.pack_mlp_embedding (fp32 stages + split section).  attn_mode != 0: one launch on the fp16
 * split (k_mlpemb_h); attn_mode 0: three fp32-MFMA launches through the scratch arrays tmp1 / tmp2 [rows][128]. */
int infgen_mlp_embedding(const float* X, int ldx, int rows, int K0, const float* pack, float* tmp1, float* tmp2,
                         float* Y, int ldy, void* stream);
/* row-wise LayerNorm over 128 columns (torch.nn.LayerNorm, eps 1e-5); gamma == NULL: affine-free */
int infgen_layernorm(const float* X, int rows, const float* gamma, const float* beta, float* Y, void* stream);
int infgen_fourier_embed(const float* raw, int n_dims, const int* count_dev, int e_cap, const float* pack,
                         const float* cat, int ldcat, float* out, int ldo, int normalize, void* stream);
/* FourierEmbedding whose LAST continuous input only takes the values 0, -1, .., -31 (the time gap of the temporal edges):
 * infgen_fourier_last_dim_table writes table[32][128], row k = mlps[n-1](-k) without its bias, with the arithmetic of the
 * current gemm_terms; infgen_fourier_embed_tab evaluates dims 0 .. n-2 per row and adds row (int)(-raw[e][n-1]) of the table
 * (same result as infgen_fourier_embed up to the fp32 summation order of the per-dim branches).  Split kernel only. */
int infgen_fourier_last_dim_table(const float* pack, int n_dims, float* table, void* stream);
int infgen_fourier_embed_tab(const float* raw, int n_dims, const int* count_dev, int e_cap, const float* pack,
                             const float* table, float* out, int ldo, int normalize, void* stream);
/* arithmetic of infgen_fourier_embed: 1 (default) = fp16 MFMA with a three-term hi/lo split of both operands and fp32
 * accumulation (operands to 2^-23, round to nearest; measured at least as close to fp64 as mode 0: tests/test_precision_gpu.py; 5.3x the
 * fp32 matrix rate), 0 = fp32-input MFMA.  Process-wide default (InfgenOptions.fourier_mode per context / thread). */
int infgen_set_fourier_mode(int mode);
/* the switch for infgen_attn_pre / infgen_attn_post / infgen_attn_post_pre: 0 fp32 MFMA, 1 fp16 split, 2 (default) by
 * row count (split from ~10 k rows, where its one-workgroup-per-CU tiles fill the chip) */
int infgen_set_attn_mode(int mode);
int infgen_attn_pre(const float* X, int rows, const float* pack, int use_src_ln,
                    float* Q, float* U, float* K, float* V, void* stream);
int infgen_edge_attn(int rows, const float* Q, const float* U, const float* Ksrc, const float* Vsrc,
                     const int* off, const int* cnt, const int* src, const float* rhat,
                     float* AGG, float* Z, float* SIG, void* stream);
/* The edge side of one sublayer for 16-row tiles with the absorbed query U and the positional aggregate Z kept on chip
 * (k_edge_fused): u = q W'_kr on the matrix pipe -> LDS, the edge loop of infgen_edge_attn, then
 * AGG = sum_e a_e v_src + W'_vr z + b' sigma on the matrix pipe.  `pack` is the layer's attention pack; the node-side
 * entries that follow take this AGG with has_pos = 0 and no Z / SIG / U.  Replaces, like infgen_edge_attn, the reference's
 * MessagePassing.propagate + softmax (infgen/modules/layers.py:78-92,109).  infgen_set_edge_fuse(0) makes
 * infgen_decode_layers fall back to the unfused sequence (default 1). */
int infgen_edge_attn_fused(int rows, const float* Q, const float* pack, const float* Ksrc, const float* Vsrc,
                           const int* off, const int* cnt, const int* src, const float* rhat,
                           float* AGG, void* stream);
/* The same two operators with the normalised relative-position rows in a packed 24-bit form: per row 128 x 16 bit (bits 31..16 of
 * the fp32 values) followed by 128 x 8 bit (bits 15..8), 384 bytes, values rounded to nearest even at bit 8 (relative error 2^-17).
 * infgen_fourier_embed_r24 (normalize = 1, no categorical sum; split Fourier kernel only, i.e. infgen_set_fourier_mode != 0) writes
 * e_cap rows of 384 bytes to `out`; infgen_edge_attn_fused_r24 reads them.  infgen_decode_layers uses the form for its own sets. */
int infgen_fourier_embed_r24(const float* raw, int n_dims, const int* count_dev, int e_cap, const float* pack, void* out, void* stream);
int infgen_edge_attn_fused_r24(int rows, const float* Q, const float* pack, const float* Ksrc, const float* Vsrc,
                               const int* off, const int* cnt, const int* src, const void* rhat24, float* AGG, void* stream);
/* Which of the two row formats infgen_decode_layers / infgen_rollout_run keep their own edge sets' rhat rows in between the Fourier
 * and the edge launches: 0 (default) fp32 - the reference's arithmetic (infgen/modules/layers.py:61-113 is fp32 end to end) -,
 * 1 the packed 24-bit rows above (-25 % of the rhat bytes, ~1 % of a rollout; outside the fp32 contract, a named secondary leg of
 * bench.py).  Process-wide default; a context with opts.use != 0 takes InfgenOptions.rhat_format. */
int infgen_set_rhat_format(int format);
int infgen_set_edge_kernel(int kernel);
int infgen_set_edge_fuse(int mode);
/* the process-wide defaults (what the infgen_set_* functions edited so far), e.g. to seed a context's own InfgenOptions */
int infgen_get_options(InfgenOptions* out);
/* Re-entrancy of the OPERATOR-level entries (infgen_fourier_embed, infgen_attn_*, infgen_edge_attn*, infgen_heads, infgen_linear ...):
 * they take their switches from the calling THREAD's option block when one is installed, else from the process-wide defaults.
 * infgen_thread_options(o) installs a copy of *o for the calling thread (o == NULL removes it); a rollout-level entry called
 * with a context whose opts.use != 0 still takes the context's block.  Two engines driven from two host threads therefore never
 * see each other's settings, whatever the infgen_set_* defaults are (infgen_amd/engine.py installs the engine's block around its
 * prologue).  infgen_get_effective_options returns what an operator-level call from this thread would use right now. */
int infgen_thread_options(const InfgenOptions* o);
int infgen_get_effective_options(InfgenOptions* out);
/* diagnostics: resident workgroups per CU the runtime reports for k_edge_fused; a plain streaming read of n_bytes with 8 or
 * 16 bytes per lane for calibrating rocprofv3 FETCH_SIZE (tools/calibrate_fetch.sh; out: 2048 floats) */
int infgen_edge_fused_occupancy(void);
int infgen_debug_stream_read(const float* p, unsigned long long n_bytes, int width, float* out, void* stream);
/* edges per trip of k_edge_fused's edge loop (their K / V / rhat rows are requested together): 4, 6 (default) or 8 */
int infgen_set_edge_loop(int variant);
/* 1: infgen_decode_layers runs the Fourier embeddings of the map and agent edge sets on an internal side stream, overlapped
 * with the first temporal / map sublayers on the caller's stream (joined with events before their first use) */
int infgen_set_overlap(int mode);
/* 1 (default; INFGEN_LAYERS_P=0 in the environment: off): launches of up to 256 16-row groups run ALL 18 sublayers of a decode step
 * in one launch of k_layers_p (one resident workgroup per group, wave = feature tile; the scene's groups meet at a counter before
 * each agent sublayer) instead of 36 launches of k_edge_fused + k_attn_hs - same operators (infgen/modules/layers.py:61-113),
 * rounding-level differences only.  Needs fused edge attention (infgen_set_edge_fuse != 0) and the split GEMM kernels; otherwise
 * the per-sublayer launches run (a row-group list of an insertion context is ignored by this kernel: it visits every group).
 * Process-wide default like the other infgen_set_*: a context with opts.use != 0 takes InfgenOptions.layers_p instead.
 * Concurrency: a launch never exceeds the workgroups the CURRENT device keeps resident for this kernel (occupancy query x CUs; also on
 * partitions with fewer CUs), the launches of different streams of one process are ordered behind each other by the library (an event
 * recorded behind every launch on its own stream - no stream handle is kept), and the wait at the counters is bounded only by a
 * trap after 2^24 polls (tens of seconds; INFGEN_LP_SPIN_LIMIT) - contexts may run concurrently on several streams or host threads,
 * next to other kernels (tests/test_rollout_gpu.py).
 * mode 2: the same through hipLaunchCooperativeKernel (device-wide cooperative queue: also safe next to ANOTHER PROCESS that runs
 * such kernels on the same GPU; ~25 us more per launch; a runtime that refuses the launch gets the per-sublayer launches from
 * then on).  (A stream that is being captured into a HIP graph takes a plain launch with a bounded wait: graph replay is an
 * opt-in mode whose caller owns the GPU.)
 * infgen_layers_p_capacity: workgroups one such launch may have on the current device (0: the kernel is unavailable here). */
int infgen_set_layers_p(int mode);
int infgen_layers_p_capacity(void);
/* same with the kernel variant forced: wide = 1 -> one 8-wave workgroup per destination (long edge lists, few rows),
 * wide = 0 -> one wave per destination; infgen_edge_attn picks wide when rows <= 256 */
int infgen_edge_attn_mode(int rows, const float* Q, const float* U, const float* Ksrc, const float* Vsrc,
                          const int* off, const int* cnt, const int* src, const float* rhat,
                          float* AGG, float* Z, float* SIG, int wide, void* stream);
int infgen_attn_post(float* X, int rows, const float* pack, const float* AGG, const float* Z, const float* SIG,
                     int has_pos, void* stream);
/* infgen_attn_post followed, on the same rows, by the NEXT layer's infgen_attn_pre (one launch) */
int infgen_attn_post_pre(float* X, int rows, const float* pack, const float* AGG, const float* Z, const float* SIG,
                         int has_pos, const float* next_pack, float* nQ, float* nU, float* nK, float* nV, void* stream);
int infgen_heads(const float* X, int rows, const float* tok_pack, const float* st_pack, int token_size,
                 float* logits, int* next_token, int* next_state, void* stream);
/* infgen_heads plus token_logprob [rows] = log_softmax(logits[row])[next_token[row]] (full softmax, fp32, max-subtracted, fixed
 * summation order).  Where the split kernel runs (attn_mode 1, or 2 beyond 10240 rows) the log-sum-exp is fused into it and
 * logits may be NULL; elsewhere k_heads writes the caller's logits [rows][token_size] (NULL: refused) and infgen_token_logprob
 * reads them.  next_token / next_state / logits are bitwise those of infgen_heads. */
int infgen_heads_logprob(const float* X, int rows, const float* tok_pack, const float* st_pack, int token_size,
                         float* logits, int* next_token, int* next_state, float* token_logprob, void* stream);
/* out[row] = logits[row][token[row]] - logsumexp(logits[row]) over n columns (one wave per row); 0 where token[row] < 0 */
int infgen_token_logprob(const float* logits, int rows, int n, const int* token, float* out, void* stream);
/* infgen_heads with next_token drawn by top-k sampling: the k (1..16, <= token_size) best logits of the row in (value descending,
 * column ascending) order, inverse CDF over p[j] = exp(v[j] - v[0]) with uniform[row] in [0, 1) - infgen_sample_topk's order and
 * arithmetic, so the tokens equal infgen_heads + infgen_sample_topk bit for bit.  Optional outputs (NULL: not computed):
 * logits [rows][token_size]; token_logprob [rows], the FULL-softmax log-probability of the sampled token; sample_logprob [rows], its
 * log-probability under the re-normalised top-k distribution, (v_pick - v_0) - log(sum_j p[j]).  Where
 * infgen_heads_sample_fused(attn_mode, rows, k) holds this is ONE launch of the split heads kernel, which keeps a running top-k in
 * registers and stores no logit unless asked; elsewhere it is infgen_heads into the caller's logits (NULL: refused, "needs a logits
 * buffer"), infgen_sample_topk_logprob and infgen_token_logprob.  k == 1 is the arg-max (sample_logprob 0). */
int infgen_heads_sample(const float* X, int rows, const float* tok_pack, const float* st_pack, int token_size, int k,
                        const float* uniform, float* logits, int* next_token, int* next_state, float* token_logprob,
                        float* sample_logprob, void* stream);
/* the same with temperature and nucleus truncation (InfgenSampling above; sampling == NULL: infgen_heads_sample).  Still one launch
 * where infgen_heads_sample_fused holds - the rule does not look at the parameters - and the same tokens and sample_logprob, bit for
 * bit, as infgen_heads + infgen_sample_topk_ex.  token_logprob stays the full softmax at temperature 1. */
int infgen_heads_sample_ex(const float* X, int rows, const float* tok_pack, const float* st_pack, int token_size, int k,
                           const float* uniform, const InfgenSampling* sampling, float* logits, int* next_token, int* next_state,
                           float* token_logprob, float* sample_logprob, void* stream);
/* infgen_heads_sample_ex under a token mask (the five parameters described above InfgenRollout; an inactive mask: infgen_heads_sample_ex, bit for bit).
 * k <= 1 is the masked arg-max (uniform may then be NULL; sample_logprob 0).  The by-size rules below do not look at the mask: where
 * infgen_heads_sample_fused / infgen_heads_logprob_fused hold this is still one launch without logits in memory. */
int infgen_heads_sample_mask(const float* X, int rows, const float* tok_pack, const float* st_pack, int token_size, int k,
                             const float* uniform, const InfgenSampling* sampling, const uint32_t* mask_bits, int mask_n_sets,
                             const int* mask_row, const int* mask_type, const int* type, float* logits,
                             int* next_token, int* next_state, float* token_logprob, float* sample_logprob, void* stream);
/* 1 where top-k sampling with beam k runs inside the split heads kernel: attn_mode 1, or >= 2 beyond INFGEN_Q_ATTN_SPLIT_ROWS
 * rows, and 2 <= k <= INFGEN_Q_HEADS_SAMPLE_K.  The one statement of the rule: infgen_heads_sample, infgen_decode_step and the
 * engine's decision to allocate logits_scratch all go through it. */
int infgen_heads_sample_fused(int attn_mode, int rows, int k);
/* 1 where the greedy step's token log-probability comes out of the split heads kernel (infgen_heads_logprob's one launch, no logits
 * in memory): attn_mode 1, or >= 2 beyond INFGEN_Q_ATTN_SPLIT_ROWS rows.  The greedy counterpart of infgen_heads_sample_fused. */
int infgen_heads_logprob_fused(int attn_mode, int rows);
/* the map encoder's token_predict_head (infgen/modules/map_decoder.py:119-121) on the rows gather[k] (k < n) of X [..][ldx]:
 * logits [n][token_size] (raw, fp32) and top_idx [n][10] (int64), the indices of the 10 largest logits in descending order (softmax
 * is monotone), equal values lower index first.  pack = infgen_amd.packing.pack_mlp_layer of the head; token_size must be 1024.
 * Arithmetic as infgen_heads: the split kernel (one launch, ranking fused) under gemm_terms 1 / 2 and from the attn_mode row count,
 * else fp32 MFMA through hidden [n][128] (scratch, always pass it). */
int infgen_map_token_head(const float* X, int ldx, const int* gather, int n, const float* pack, int token_size,
                          float* hidden, float* logits, long long* top_idx, void* stream);
/* out[k][:] = tab0[idx0[k]] + ((tab1[idx1[k]] + tab2[idx2[k]]) + tab3[idx3[k]]), rows of 128 floats, int64 indices (clamped to
 * the table sizes n0 .. n3): the map-token embedding plus the sum of its three nn.Embedding rows in one pass
 * (infgen/modules/map_decoder.py:87-89 and the token table of :70-86), in torch's summation order */
int infgen_embedding_sum4(const float* tab0, const long long* idx0, int n0, const float* tab1, const long long* idx1, int n1,
                          const float* tab2, const long long* idx2, int n2, const float* tab3, const long long* idx3, int n3,
                          int rows, float* out, void* stream);
/* compacted CSR: `total` (device int) receives the edge count; rows whose edges would exceed `cap`
 * get cnt = 0 and the caller must retry with a larger buffer when *total > cap */
int infgen_map_graph(int S, int M_cap, const int* n_map, const float* pos, const float* orient, float radius,
                     int max_nbr, int* off, int* cnt, int* src, float* raw, int* total, int cap, void* stream);

/* checks a freshly built context (sizes, required pointers) and examines its attention packs' headers (64-byte device -> host
 * copies: synchronous; k_layers_p needs the LayerNorm bounds of header slots 10..13, version slot 14 - contexts whose packs lack
 * them take the per-sublayer launches).  Optional: without it a pack is examined when its device address is first seen, which
 * goes wrong if that address held another pack earlier in the process. */
int infgen_rollout_validate(const InfgenRollout* r);
int infgen_build_edges(const InfgenRollout* r, int c, int edgeless, void* stream);
int infgen_integrate(const InfgenRollout* r, int t, void* stream);
int infgen_raw_feature(const InfgenRollout* r, int col, void* stream);
/* the same for the rows row_list[k] with row_mask[k] != 0 only (k < n; the rows a sub-loop iteration of the insertion appended) */
int infgen_raw_feature_rows(const InfgenRollout* r, int col, const int* row_list, const int* row_mask, int n, void* stream);
int infgen_decode_layers(const InfgenRollout* r, int c, int edgeless, void* stream);
int infgen_decode_step(const InfgenRollout* r, int t, void* stream);
/* steps t0 .. t1-1 back to back (one host call per rollout) */
int infgen_rollout_run(const InfgenRollout* r, int t0, int t1, void* stream);
/* The split mode of infgen_rollout_run: a large batch runs as two halves of S / 2 scenes on two streams of the
 * library's own, forked from `stream` at entry and joined to it at exit - the caller sees one ordered call and, per scene, the same
 * kernels on the same rows, bit for bit.  The second half's step starts INFGEN_SPLIT_OFFSET sublayers (two launches each; default 4, a
 * quarter step of six layers; 0: no phase control) behind the first half's.  INFGEN_SPLIT_HALVES: 0 never; 1 (default) when each half keeps every
 * by-size kernel choice of the whole batch (more than 10,240 rows per half, no k_layers_p), S is even and its middle no inside of a
 * copy group (map_scene), without scenario insertion, a token-mask handle, tap_x or per-kernel profiling, and `stream` is not being
 * captured into a graph; 2: the same without the size rule (tests).  The halves own their share of the three edge buffers and their own
 * totals, summed into the context's after the last step (a half that overflows its share reports more than the whole capacity).
 * infgen_set_overlap's side stream is not used by a split rollout.  infgen_split_stats: calls of infgen_rollout_run that took the
 * split / the single-stream path since the library was loaded (either pointer may be NULL). */
int infgen_split_stats(int* split_runs, int* single_runs);
/* closed-loop sessions: the commands of decode step t for the rows flagged in r->replay_row, written into column 2 + t of the plan
 * the step's infgen_integrate forces on them (r->teacher_token / teacher_state; refused without them or without replay_row); call it
 * in front of infgen_decode_step(r, t).  kind 0: cmd_token [S][A_cap] ids (state valid; ids beyond the vocabulary are clamped).
 * kind 1: cmd_pose [S][A_cap][3] = x, y, heading in the world frame - the row's box (shape [S][A_cap][3] = length, width, height)
 * at that pose is matched against the last contour of every token of the row's type, moved by the row's stored pose with
 * infgen_integrate's arithmetic; cost = sum of the four corner distances, first minimum wins.  With r->teacher_pos / teacher_head the
 * stored pose becomes the commanded one, without them it is the matched token's integration.  cmd_mask (optional [S][A_cap]): 0 = no
 * command, the row leaves the scene (state invalid); a row whose stored state is invalid stays invalid.  cmd_cost (optional
 * [S][A_cap]): the winning cost (0 for token commands).  Rows without a flag, rows >= n_agents[s] and every other column are not
 * touched.  The pointers that r declares const are written here (the plan belongs to the caller).  A_cap need not be a multiple of 32. */
int infgen_command_rows(const InfgenRollout* r, int t, int kind, const int* cmd_token, const float* cmd_pose,
                        const unsigned char* cmd_mask, const float* shape, float* cmd_cost, void* stream);

/* branching rollouts: BRANCHING, "scene slot s becomes a clone of slot p as of the boundary in front of decode step t" - what
 * beam pruning and sequential Monte Carlo over the copies of a scene need (k_branch_scenes: one launch, no host read); the way back in
 * time that MPC and tree search with backtracking need is "snapshots" below.
 * infgen_branch_scenes: parent is a device int32 array [S].  For every agent-side scene s with p = parent[s] != s, slot s receives slot
 * p's rollout state as it stands between decode step t - 1 and decode step t, 0 <= t <= steps (= T - 2):
 *   copied   the per-scene [T][A_cap] blocks of pos (x 2), head, state, token, grid, tmask, imask, catflag, and bos [A_cap];
 *            every ring slot of ringK[l] / ringV[l], l < num_layers (A_cap x 128 floats per ring slot and scene);
 *            the scene's rows of X - the fused raw feature of column 2 + t the previous step's tail left; nothing recomputes it;
 *            pred_traj / pred_head / pred_state;
 *            the slices [0, t) of token_logprob, sample_logprob and (store_logits) logits, where those pointers are given.
 *   kept     what configures a slot and is not history: sample_u, sample_temp_row, the token mask's selectors and tables, replay_row,
 *            the plan arrays teacher_* (past plan columns are not read again, future ones are the slot's own commands), the collision
 *            and road buffers (rebuilt every step from the copied poses), the routes, their records and the route buffers (route_bits,
 *            count and progress are rebuilt every step too), type / n_agents and the map side (equal inside a copy
 *            group).  A clone therefore diverges from its parent at the next draw or command.  Scratch is not touched.
 *   parent   source and destination belong to one COPY GROUP, the same map-side scene: map_scene[s] == map_scene[p] (map_scene NULL:
 *            every scene is its own group, only the identity is valid); sources are fixed points, parent[parent[s]] == parent[s] - no
 *            slot is read and written in one launch, so the gather runs in place.  An entry that is out of range, in another group
 *            or no fixed point is treated as parent[s] = s and counted into *n_bad (optional device int, zeroed by the call first);
 *            nothing outside the layout is read for any content of parent, and the library never dereferences parent on the host.
 * Refused: t out of range, a NULL parent, a context with scenario insertion (first_new != NULL: row counts, types and shapes differ
 * between the copies and part of the bookkeeping lives in host lists - branching such a context is left out).
 * infgen_resample_parents: arbitrary ancestor indices [S0 * copies] (global slot indices inside the slot's own group, as a resampler
 * produces them; one outside its group counts as the slot itself) -> a valid parent vector [S0 * copies]: a slot that is named at
 * least once keeps itself; the slots nobody names, in ascending order, receive the surplus - ancestor j's count[j] - 1 extra copies, in
 * ascending j.  The multiset of ancestors per group is preserved and the result is deterministic.  One workgroup per group;
 * 1 <= copies <= 1024, else refused. */
int infgen_branch_scenes(const InfgenRollout* r, int t, const int* parent, int* n_bad, void* stream);
int infgen_resample_parents(const int* ancestor, int S0, int copies, int* parent, void* stream);

/* snapshots: SNAPSHOTS, "the decode state of scene slot s as of the boundary in front of decode step t, kept outside the context and put
 * back later" - the way back in time: an MPC planner's look-ahead, tree search with backtracking, counterfactual re-runs
 * (k_snapshot_scenes<RESTORE>: one launch per call, no host read).  Without scenario insertion a decode step is a function of the
 * context and t, so a restored slot continues exactly as the saved one would have.
 * A snapshot ENTRY holds exactly what infgen_branch_scenes copies (its "copied" list, the same segment table):
 *   the per-scene [T][A_cap] blocks of pos (x 2), head, state, token, grid, tmask, imask, catflag, and bos [A_cap];
 *   every ring slot of ringK[l] / ringV[l], l < num_layers; the scene's rows of X; pred_traj / pred_head / pred_state;
 *   the slices [0, t) of token_logprob, sample_logprob and (store_logits) logits, where those pointers are given;
 *   the scene's [steps][8] step-score block, where the context scores ("step scores").
 * and nothing of its "kept" list (uniforms, temperatures, mask selectors and tables, replay flags, plans, collision and road buffers,
 * routes, route records and route buffers, scratch): a restored slot runs under the configuration the context has THEN, which is what a planner varies between two tries.
 * Layout: the segments in table order (the order above; absent buffers take no room), each segment as its blocks per scene - one for
 * the scene arrays, X and pred_*, `ring` for a ring, t for a log - every block starting on a 16-byte boundary (a block of b bytes takes
 * (b + 15) & ~15; the library's own layouts have b % 16 == 0).  The bytes between a block's end and the boundary are written as 0.
 * infgen_snapshot_bytes: host only, launches nothing: *bytes = the bytes of one entry at step t (a multiple of 16); returns 0 or a
 *   negative code like every entry.  Monotone in t - the bytes at t = steps are the capacity for any step.
 * infgen_snapshot_scenes: slots is a device int32 array [n], 0 <= n <= 65535; entry e (the entry_stride bytes at snap + e *
 *   entry_stride) receives slot slots[e], and head [n][4] (device int32) receives {slot, group, t, valid} with group = map_scene[slot]
 *   (map_scene NULL: the slot itself).  A slot out of range writes {slot, -1, t, 0}, moves nothing and is counted into *n_bad (optional
 *   device int, zeroed by the call first).  The context is not written.
 * infgen_restore_scenes: index is a device int32 array [S]; slot s receives entry index[s], -1 = keep.  One entry may go to several
 *   slots (fan-out: the same as a branch from the saved slot).  An entry is applied only if 0 <= index[s] < n, its head says valid,
 *   head.t == t and head.group is slot s's group; any other entry is read as -1 and counted into *n_bad.
 * Nothing outside the two layouts (the context's buffers, n entries of entry_stride bytes, head [n][4]) is read or written for any
 * content of slots, index or head, and the library never dereferences them on the host.  A context-side segment whose base, block size
 * or stride is no multiple of 16 is moved byte by byte on that side; the snapshot side is always 16-byte aligned.
 * Refused: t outside 0..steps, NULL arrays, entry_stride below the bytes of infgen_snapshot_bytes(r, t) or no multiple of 16, snap not 16-byte aligned,
 * n outside 0..65535, a context with scenario insertion (first_new != NULL: left out for the reason branching gives).
 * Cost: an entry is dominated by the rings, 2 * num_layers * ring * A_cap * 512 bytes per slot. */
int infgen_snapshot_bytes(const InfgenRollout* r, int t, long long* bytes);
int infgen_snapshot_scenes(const InfgenRollout* r, int t, const int* slots, int n, void* snap, long long entry_stride, int* head,
                           int* n_bad, void* stream);
int infgen_restore_scenes(const InfgenRollout* r, int t, const int* index, const void* snap, long long entry_stride, const int* head,
                          int n, int* n_bad, void* stream);

/* reproducible stand-in for softmax -> topk(k) -> multinomial (agent_decoder.py:2162-2163,2194-2195): the k most
 * probable tokens, inverse-CDF over their probabilities with a caller-supplied uniform per row; 1 <= k <= min(16, n), else refused */
int infgen_sample_topk(const float* logits, int rows, int n, int k, const float* uniform, int* token, void* stream);
/* the same, plus sample_logprob [rows] (optional): the pick's log-probability under the re-normalised top-k distribution */
int infgen_sample_topk_logprob(const float* logits, int rows, int n, int k, const float* uniform, int* token,
                               float* sample_logprob, void* stream);
/* the same with temperature and nucleus truncation (InfgenSampling above; NULL: infgen_sample_topk_logprob); nucleus (optional,
 * [rows]): the nucleus size m of every row (k where top_p = 1, 1 on a greedy row) */
int infgen_sample_topk_ex(const float* logits, int rows, int n, int k, const float* uniform, const InfgenSampling* sampling,
                          int* token, float* sample_logprob, int* nucleus, void* stream);
/* the same under a token mask (the five parameters described above InfgenRollout; inactive: infgen_sample_topk_ex, bit for bit): banned columns
 * are never picked and the draw is over min(k, allowed) entries; n must be a multiple of 32 */
int infgen_sample_topk_mask(const float* logits, int rows, int n, int k, const float* uniform, const InfgenSampling* sampling,
                            const uint32_t* mask_bits, int mask_n_sets, const int* mask_row, const int* mask_type, const int* type,
                            int* token, float* sample_logprob, int* nucleus, void* stream);
/* registers a token mask for rollout contexts -> its handle (>= 1; InfgenRollout.token_mask), or -1 (infgen_last_error).  The
 * pointers are kept, not the contents: table and selectors stay the caller's device buffers, and rewriting them changes what the
 * next step - or the next replay of a captured graph - reads.  mask_type (three host ints, NULL = all -1) is copied.  type == NULL:
 * the context's own row types.  The token_size-dependent checks happen when a context uses the handle (infgen_rollout_validate).
 * infgen_token_mask_destroy frees the slot (0 on success); a context must not name a destroyed handle. */
int infgen_token_mask_create(const uint32_t* mask_bits, int mask_n_sets, const int* mask_row, const int* mask_type, const int* type);
int infgen_token_mask_destroy(int handle);
/* test and diagnostic entry, host only, launches nothing: copies out the library's step-rider block - the static mask as the kernels
 * take it, then the collision, road, score and route configurations, in that order - that a context with row types `type` and this
 * token_size would run under `handle` (0: no handle, the block of a context without token_mask).  -> the block's size in bytes, or a
 * negative code; capacity below that size is refused.  The layout is the library's own and may grow at its end. */
int infgen_token_mask_riders(int handle, const int* type, int token_size, void* out, int capacity);

/* collision-aware decoding: COLLISION MASKS, the allowed-token sets of one decode step computed from the agents' boxes (k_collision_mask).
 * At decode step t the current column is c = hist_columns - 1 + t (= 1 + t).  A row i of scene s is IN THE SCENE at column c when
 * i < n_agents[s], i < first_new[s] where that array is given (rows scenario insertion appended inside this step), and state[c][i] is
 * not invalid (0).  For such a row:
 *   candidate box of token k   the last contour of vocab[type[i]][k], four corners in the agent frame: its centre is the mean of the
 *       corners, its heading atan2(c0 - c3), front-left minus rear-left (the rule of infgen_integrate / infgen_command_rows); rotated by
 *       head[c][i] and moved by pos[c][i].  The box is the row's OWN length x width, shape[i] = (length, width, height) - box_contour's
 *       convention -, not the vocabulary's template box.
 *   obstacles   every other row j != i of the scene that is in the scene at column c.  predict = 0: at its pose of column c.
 *       predict = 1 and j also in the scene at column c - 1 (state[c - 1][j] not invalid): constant velocity, position
 *       2 pos[c] - pos[c - 1], heading head[c] + wrap(head[c] - head[c - 1]) (the orientation of a box does not depend on the branch of
 *       wrap); otherwise the pose of column c.  Half length and half width are each enlarged by `margin` metres.
 *   overlap   the separating-axis test of two oriented rectangles over their four axes: sep = the maximum over the axes of
 *       |projected centre distance| - the sum of the projected half extents; the boxes overlap iff sep < 0.  Evaluated in row i's
 *       frame - pos[c][i] is subtracted from the obstacle's centre first - so magnitudes stay at tens of metres wherever the scene
 *       lies in the world (fp32 throughout; a pair with |sep| below ~1e-4 m may fall either way).
 *   result   set(i) = base(i) AND NOT collides(i), collides(i) = the tokens whose candidate box overlaps an obstacle; base(i) is the
 *       static set the token mask's selectors name (mask_row, then mask_type[type]; all tokens when neither names one).  An empty
 *       result is replaced by base(i): the heads kernels never meet an empty set.  out_count[i] (optional) is the number of allowed
 *       tokens BEFORE that fallback - 0 says it was taken.
 * Rows that are not in the scene at column c, and padding rows, get base(i) (out_count: its size).  Replayed, commanded and
 * teacher-forced rows keep their plan's tokens, as under a static mask.
 * Left out on purpose: the contours 0..4 inside the 0.5 s step (only its end is tested); the planned next pose of replayed rows (they
 * are obstacles like every other row, at their current or extrapolated pose); map geometry (the road masks below); rows scenario insertion appends inside
 * step t are obstacles, and get sets, from step t + 1 on - during step t they take their type's static set, as before.
 *
 * infgen_collision_end_poses: end_pose [3][token_size][4] = (dx, dy, cos dtheta, sin dtheta) of every token's last contour in the agent
 * frame, followed by four floats: the largest displacement sqrt(dx^2 + dy^2) of the three types, and 0 - 12 token_size + 4 floats,
 * 16-byte aligned, computed once per vocabulary ([3][token_size][6][4][2]).
 * infgen_collision_mask: one launch writes out_bits [S * A_cap][token_size / 32] (16-byte aligned) and out_count (optional).  The scene
 * arrays are laid out like InfgenRollout's ([S][T][A_cap]); A_cap need not be a multiple of 32.  The base is a token mask's first
 * four values with the rows' own `type` (mask_bits NULL: every token).  first_new: optional [S].
 * infgen_token_mask_collision: attaches a collision configuration to a registered token mask (one created with mask_bits NULL and
 * mask_n_sets 0 has the base "every token"): infgen_decode_step of a context that names the handle then launches k_collision_mask for
 * the step's column in front of the heads launch - base = the handle's static mask, out_bits = dyn_bits [S * A_cap][token_size / 32],
 * first_new = the context's - and hands the heads route dyn_bits with the identity selector identity_row ([S * A_cap], entry i = i) and no
 * per-type set.  The pointers are kept, not the contents (static device buffers: a captured graph replays what they hold then).
 * dyn_bits NULL detaches: the launches and the bits are those of the static mask again.
 * Refused: margin negative or not finite, predict outside {0, 1}, a missing shape array / end-pose table / output, a token_size that
 * is no multiple of 32 or exceeds 4096, A_cap beyond INFGEN_Q_MAX_AGENTS, a misaligned table. */
int infgen_collision_end_poses(const float* vocab, int token_size, float* end_pose, void* stream);
int infgen_collision_mask(const float* pos, const float* head, const int* state, const int* n_agents, const int* first_new,
                          const int* type, const float* shape, int S, int A_cap, int T, int c, const float* end_pose, int token_size,
                          int predict, float margin, const uint32_t* mask_bits, int mask_n_sets, const int* mask_row,
                          const int* mask_type, uint32_t* out_bits, int* out_count, void* stream);
int infgen_token_mask_collision(int handle, uint32_t* dyn_bits, const int* identity_row, const float* shape, const float* end_pose,
                                int predict, float margin, int* count);

/* road-aware decoding: ROAD MASKS, the allowed-token sets of one decode step computed from the map's road-edge segments (k_road_mask).
 * Step column c = 1 + t, IN THE SCENE, first_new, base(i) and the fallback mean what they mean for the collision masks above; fp32
 * throughout, no fused multiply-add.
 *   road segments   row-scene s of an engine with `copies` uses the segments of map scene s / copies.  From the map: every map token
 *       m < n_map with map_type[m] == 12 (EDGE) and 0 <= map_tok[m] < n_token contributes `detail` (1, 2, 5 or 10) chords of its
 *       vocabulary polyline map_vocab[map_tok[m]] (11 points in the token frame), joining the points 0, 10 / detail, ..., 10, each
 *       rotated by map_orient[m] and anchored at map_pos[m]; a token of another type, or with a token id outside the vocabulary,
 *       contributes nothing.  Explicit: segments [S0][E][4] = (x0, y0, x1, y1) in world coordinates, the first n_segments[s] of scene s.
 *   record   8 floats, 16-byte aligned: anchor x, y - an exact copy of an input world coordinate, map_pos[m] or the segment's p0 -,
 *       the offset of the segment's midpoint from the anchor, cos and sin of the segment's direction (p1 - p0) / L, the half length
 *       L / 2 and the enclosing radius L / 2.  A segment with L == 0 or a non-finite coordinate is the record (0, 0, 0, 0, 1, 0, 0, -1):
 *       radius -1, never an obstacle.  The kernel forms (anchor - pos[c][i]) + offset: world coordinates enter through an exact
 *       difference only, the rule of (centre - pos) + step above.  Records are compacted per scene - tokens in order, a token's chords
 *       in order -, n_records[s] of them, records [S0][rec_cap][8]; what exceeds rec_cap is dropped (callers size rec_cap from a count).
 *   obstacle rectangle   centre the segment's midpoint, heading its direction, half extents (L / 2 + margin, margin).
 *   candidate shapes of token k for row i   the END BOX: the candidate box of the collision masks (the last contour's centre and heading,
 *       the row's own length x width).  The PATH RECTANGLE (sweep = 1): centre half the end displacement (dx, dy) / 2, heading that of
 *       (dx, dy), half extents (|d| / 2, the row's half width); skipped when |d| == 0.
 *   overlap   the four-axis separating-axis value sep < 0 of the collision masks, in row i's frame.  Token k is OFF-ROAD for row i iff
 *       its end box or its path rectangle overlaps an obstacle rectangle of the scene that row i does not already STRADDLE: a segment
 *       whose obstacle rectangle overlaps the row's current box (the pose of column c, own extents) is ignored for that row in that step.
 *   rows   the rule applies to the rows in the scene at column c whose agent type ty (0 vehicle, 1 pedestrian, 2 cyclist; others
 *       count as 0) has types[ty] != 0.  Every other row - not in the scene, padding, >= first_new[s], a type switched off - keeps base(i).
 *   result   set(i) = base(i) AND NOT offroad(i); an empty result is replaced by base(i); out_count[i] (optional) is the size before
 *       that fallback.
 * infgen_road_records_from_map / infgen_road_records_from_segments: the record table of S0 distinct scenes, once per reload.
 * infgen_road_paths: paths [3][token_size][4] = (cos, sin of the end displacement's direction, |d| / 2, 0) - (1, 0, 0, 0) where
 * |d| == 0 - from the end-pose table of infgen_collision_end_poses, which also holds the largest displacement per type.
 * infgen_road_mask: one launch writes out_bits [S * A_cap][token_size / 32] and out_count (optional); the scene arrays as for
 * infgen_collision_mask, S a multiple of copies; the base is a token mask's first four values with the rows' own `type`.
 * infgen_token_mask_road: attaches a road configuration to a registered token mask, as infgen_token_mask_collision does:
 * infgen_decode_step then launches k_road_mask in front of the heads launch.  With a collision configuration on the same handle
 * k_collision_mask runs first, exactly as without this one, and the road kernel's base is its dyn_bits read through the identity
 * selector: set = collision set AND NOT offroad, an empty one replaced by the collision set.  The heads read road_bits.  The pointers
 * are kept, not the contents.  road_bits NULL detaches.
 * Refused: margin negative or not finite, sweep outside {0, 1}, detail outside {1, 2, 5, 10}, copies < 1, a missing table, a
 * token_size that is no multiple of 32 or exceeds 4096, a misaligned table. */
int infgen_road_records_from_map(const float* map_pos, const float* map_orient, const long long* map_type, const long long* map_tok,
                                 const int* n_map, int S0, int M_cap, const float* map_vocab, int n_token, int detail, float* records,
                                 int rec_cap, int* n_records, void* stream);
int infgen_road_records_from_segments(const float* segments, const int* n_segments, int S0, int E, float* records, int rec_cap,
                                      int* n_records, void* stream);
int infgen_road_paths(const float* end_pose, int token_size, float* paths, void* stream);
int infgen_road_mask(const float* pos, const float* head, const int* state, const int* n_agents, const int* first_new, const int* type,
                     const float* shape, int S, int A_cap, int T, int c, const float* end_pose, const float* paths, int token_size,
                     const float* records, const int* n_records, int rec_cap, int copies, int sweep, float margin, const int* types,
                     const uint32_t* mask_bits, int mask_n_sets, const int* mask_row, const int* mask_type, uint32_t* out_bits,
                     int* out_count, void* stream);
int infgen_token_mask_road(int handle, uint32_t* road_bits, const int* identity_row, const float* shape, const float* end_pose,
                           const float* paths, const float* records, const int* n_records, int rec_cap, int copies, int sweep,
                           float margin, const int* types, int* count);

/* route-following decoding: ROUTE MASKS, the allowed-token sets of one decode step computed from the rows' own routes (k_route_mask):
 * where the collision and road masks say where a row may not go, this one says where it should - the model still decides speed, gaps
 * and lateral detail inside the corridor.  Step column c = 1 + t, IN THE SCENE, first_new, base(i) and the fallback mean what they
 * mean for the collision masks above; fp32 throughout, no fused multiply-add; world coordinates enter only through the exact
 * difference (p0 - pos[c][i]).
 *   route   row (s, i) of `copies` copies per scene reads the route of row (s / copies, i): n_points waypoints in world coordinates,
 *       routes [S0][A_cap][P][2], n_points [S0][A_cap], 0 <= n_points <= P (values outside are clamped), 2 <= P <= 32.  Longer paths
 *       are the caller's to window between steps.
 *   record   built once per (re)load by k_route_records, one per segment j (the points j, j + 1), records [S0][A_cap][P - 1][8],
 *       16-byte aligned: p0.x, p0.y (exact copies of the input), ux, uy = (p1 - p0) / L, L = sqrt(dx * dx + dy * dy), cum = the arc
 *       length in front of the segment - the live L before it, summed in segment order -, 0, 0.  A segment with L == 0, a non-finite
 *       L or p0, or an end beyond n_points is the DEAD record (0, 0, 1, 0, -1, 0, 0, 0): it is skipped and cum does not advance.
 *       total [S0][A_cap] = the sum over all live segments.  A row HAS A ROUTE iff total > 0 (fewer than two points: none).
 *   projection   a point e of the row's frame - translate by pos[c][i] first, then rotate by -head[c][i]: q0 = R(p0 - pos), u = R(ux, uy)
 *       with R(x, y) = (x ci + y si, y ci - x si) - over the live segments in order: a = min(max((e - q0) . u, 0), L),
 *       d2 = |e - q0 - a u|^2; the FIRST segment of least d2 gives s(e) = cum + a and d(e) = sqrt(d2).  s0, d0: the values of the
 *       row's current centre, e = (0, 0); s_k, d_k: those of the centre (dx, dy) of token k's END BOX (the end-pose table, the row's type).
 *   on-route   token k is ON-ROUTE iff (d_k <= corridor or d_k < d0) - the second clause lets a row that starts outside the corridor
 *       come back - and s_k >= s0 - back (the difference formed once per row).
 *   pace   0 <= pace <= 1, 0: off.  gmax = the maximum of s_k - s0 over the tokens in base(i) that are on-route.  With pace > 0 and
 *       gmax > 0 the tokens with s_k - s0 < pace * gmax (the product formed once per row) are banned too.
 *   rows   the rule applies to the rows in the scene at column c that have a route, whose agent type ty (0 vehicle, 1 pedestrian,
 *       2 cyclist; others count as 0) has types[ty] != 0 and that are not FINISHED: s0 < total - finish (the difference in fp32).  Every
 *       other row - no route, finished, not in the scene, padding, >= first_new[s], a type switched off - keeps base(i).  Replayed,
 *       commanded and teacher-forced rows keep their plan's tokens, as under any mask.
 *   result   set(i) = base(i) AND onroute(i) (AND the pace bar); an empty result is replaced by base(i); out_count[i] (optional) is
 *       the size before that fallback.  out_progress [S * A_cap][4] (optional, 16-byte aligned) = (s0, d0, total, flag): flag 1 =
 *       ruled, 2 = finished; a row in the scene with a route and its type on has s0 and d0, every other row (0, 0, total, 0).
 *       A d or s within ~1e-4 m of one of its thresholds, or two segments whose d2 tie that closely, may fall either way.
 * infgen_route_records: records and total of S0 * A_cap rows from routes and n_points.
 * infgen_route_mask: one launch writes out_bits [S * A_cap][token_size / 32], out_count and out_progress; the scene arrays as for
 * infgen_collision_mask, S a multiple of copies; the base is a token mask's first four values with the rows' own `type`.  shape is
 * the rows' [S][A_cap][3] array of the collision masks (the row skeleton reads it; the rule itself tests centres, not boxes).
 * infgen_token_mask_route: attaches a route configuration to a registered token mask, as infgen_token_mask_road does:
 * infgen_decode_step then launches k_route_mask in front of the heads launch, after k_collision_mask and k_road_mask where the
 * handle carries those: collision, then road, then route - each stage's base is the previous stage's bits read through the identity
 * selector, each stage's fallback returns the previous stage's set, and the heads read route_bits.  With no route configuration
 * attached the launches and their arguments are exactly those without this entry.  progress is rebuilt every step, like count.  The
 * pointers are kept, not the contents: records and total may be rebuilt between two steps.  route_bits NULL detaches.  Rows scenario
 * insertion appends have no route (their n_points is 0) and keep their base.
 * Refused: corridor, back or finish negative or not finite, pace outside [0, 1], P outside 2..32, copies < 1 or not dividing S, a
 * token_size that is no multiple of 32 or exceeds 4096, A_cap beyond INFGEN_Q_MAX_AGENTS, a missing or misaligned table. */
int infgen_route_records(const float* routes, const int* n_points, int S, int A_cap, int P, float* records, float* total, void* stream);
int infgen_route_mask(const float* pos, const float* head, const int* state, const int* n_agents, const int* first_new, const int* type,
                      const float* shape, int S, int A_cap, int T, int c, const float* end_pose, int token_size, const float* records,
                      const float* total, int P, int copies, float corridor, float back, float pace, float finish, const int* types,
                      const uint32_t* mask_bits, int mask_n_sets, const int* mask_row, const int* mask_type, uint32_t* out_bits,
                      int* out_count, float* out_progress, void* stream);
int infgen_token_mask_route(int handle, uint32_t* route_bits, const int* identity_row, const float* shape, const float* end_pose,
                            const float* records, const float* total, int P, int copies, float corridor, float back, float pace,
                            float finish, const int* types, int* count, float* progress);

/* signal-aware decoding: SIGNAL MASKS, the allowed-token sets of one decode step computed from the map scene's stop lines and their
 * phase at that step (k_signal_mask): a stop line is DIRECTIONAL (it bars the traffic that approaches it lawfully, never the cross or
 * oncoming traffic), TIME-VARYING (closed or open per decode step) and governs only rows that are still IN FRONT of it - three things a
 * road record is not.  Step column c = 1 + t, IN THE SCENE, first_new, base(i) and the fallback mean what they mean for the collision
 * masks above; fp32 throughout, no fused multiply-add, every sum and product in the order written here; world coordinates enter only
 * through the exact difference (m - pos[c][i]).
 *   lines   per map scene: lines [S0][K][4] = (ax, ay, bx, by) in world coordinates and n_lines [S0], 1 <= K <= 64, counts clamped to
 *       0 .. K.  a is the LEFT end and b the RIGHT end as the traffic the line stops sees them.  Row (s, i) of `copies` copies per
 *       scene reads the lines of map scene s / copies.
 *   record   built once per (re)load by k_signal_records, records [S0][K][8], 16-byte aligned: mx, my, nx, ny, half, 0, 0, 0 with
 *       d = b - a, L = sqrt(d.x * d.x + d.y * d.y), m = a + 0.5 * d (the midpoint), u = d / L, n = (-u.y, u.x) - the direction of lawful
 *       travel across the line - and half = 0.5 * L.  The rule below is stated on the record as stored: the fp32 midpoint IS the line
 *       (rounding it to a world coordinate moves the line by half an ulp at most, 0.25 mm at 5 km).  A line with L == 0, a
 *       non-finite L or a, or an index >= n_lines is the DEAD record (0, 0, 1, 0, -1, 0, 0, 0): it is skipped.
 *   phase   phase [S0][n_phase][K] bytes, n_phase >= 1: record j is CLOSED at decode step t iff phase[s0][t mod n_phase][j] != 0.  The
 *       table is cyclic: one signal cycle serves a rollout of any length.
 *   frame   as for the route masks, translate by pos[c][i] first, then rotate by -head[c][i]: with R(x, y) = (x ci + y si, y ci - x si),
 *       q = R(m - pos), v = R(n), and the line's own axis tau = (v.y, -v.x).
 *   front points   the row's own front bumper f0 = (hla, 0); token k's f_k = (dx + hla * cos_k, dy + hla * sin_k), with (dx, dy, cos_k,
 *       sin_k) the entry of the end-pose table (infgen_collision_end_poses) of the row's type, hla = shape[i][0] / 2 and
 *       hwa = shape[i][1] / 2.  For a point f: e = f - q, g(f) = (e.x * v.x + e.y * v.y) + setback, l(f) = e.x * v.y - e.y * v.x.
 *   governs   a closed live record j GOVERNS row i iff v.x >= align - the row faces the way the line is crossed - and g0 = g(f0) <= 0:
 *       its front bumper has not passed the line moved back by `setback` metres.  l0 = l(f0).
 *   runs   token k RUNS record j iff j governs the row, g_k = g(f_k) > 0 and the crossing lies on the line widened by the row's half
 *       width: | l0 * g_k - l_k * g0 | <= (half + hwa) * (g_k - g0) - the lateral offset of the point where f0 -> f_k meets the moved
 *       line, cross-multiplied: there is no division.
 *   rows   the rule applies to the rows in the scene at column c whose agent type ty (0 vehicle, 1 pedestrian, 2 cyclist; others count
 *       as 0) has types[ty] != 0.  Every other row - not in the scene, padding, >= first_new[s], a type switched off - keeps base(i).
 *       Replayed, commanded and teacher-forced rows keep their plan's tokens, as under any mask.
 *   result   set(i) = base(i) AND NOT runs(i), runs(i) = the tokens that run at least one record; an empty result is replaced by
 *       base(i) (a token that does not move the front point never runs a line, so the fallback is for rows whose base lacks every
 *       such token); out_count[i] (optional) is the size before that fallback.  out_info [S * A_cap][4] (optional, 16-byte aligned) =
 *       (gap, j, flag, 0) - what an observer, or a later car-following rule, reads: among the records that govern the row and have
 *       |l0| <= half + hwa - the line lies across the row's present lane - the one of smallest gap = -g0, ties to the smaller index; j
 *       is its index as a float, (0, -1) when there is none.  flag 1 = ruled; 2 = ruled with such a record WITHIN REACH: gap <= the
 *       largest displacement of the row's type (the end-pose table's tail).  Rows the rule does not apply to get (0, -1, 0, 0).
 *       A g, a lateral value (the crossing's offset, l0) or gap against its threshold within ~1e-4 m, or v.x within 1e-4 of align, may
 *       fall either way - the band of the route masks.
 * The kernel may skip a record whose midpoint is farther from the row than anything its tokens can make cross it (the largest
 * displacement + hla + half + hwa + setback, plus a centimetre): that changes no result.
 * infgen_signal_records: the record table of S0 distinct scenes from lines and n_lines.
 * infgen_signal_mask: one launch writes out_bits [S * A_cap][token_size / 32], out_count and out_info for decode step t (which selects
 * the phase row) at column c; the scene arrays as for infgen_collision_mask, S a multiple of copies; the base is a token mask's first
 * four values with the rows' own `type`.
 * infgen_token_mask_signal: attaches a signal configuration to a registered token mask, as infgen_token_mask_route does:
 * infgen_decode_step then launches k_signal_mask for its step t and column 1 + t AFTER k_road_mask AND BEFORE k_route_mask - collision,
 * then road, then signal, then route; each stage's base is the previous stage's bits read through the identity selector, each
 * stage's fallback returns the previous stage's set, and the heads read the last stage's bits.  Route comes last on purpose: a pace bar
 * that would push a row through a red empties the route set, and its fallback keeps the signal set.  With no signal configuration
 * attached the launches and their arguments are exactly those without this entry.  info is rebuilt every step, like count.  The
 * pointers are kept, not the contents: phase (and records) may be rewritten between two steps.  signal_bits NULL detaches.  Rows
 * scenario insertion appends keep their base in the step that appends them and are ruled from the next.  The state of a signal
 * is a function of t and the map scene alone: branching and snapshots copy nothing for it.
 * infgen_token_mask_signal_get: test and diagnostic entry, host only: copies out the handle's signal configuration (0: the empty
 * one) -> its size in bytes; infgen_token_mask_riders keeps reporting the five configurations it always did, byte for byte.
 * Left out on purpose: a closed line as a standing lead of infgen_idm_command (out_info is shaped for it); re-encoding the map's
 * light_type when a signal changes; any notion of CAUTION - the caller decides which states close a line.
 * Refused ("signal mask" in the message), on the host, before any launch: setback negative or not finite, align outside [-1, 1], K
 * outside 1..64, n_phase < 1, t < 0, copies < 1 or not dividing S, a token_size that is no multiple of 32 or exceeds 4096, A_cap
 * beyond INFGEN_Q_MAX_AGENTS, a missing or misaligned table. */
int infgen_signal_records(const float* lines, const int* n_lines, int S0, int K, float* records, void* stream);
int infgen_signal_mask(const float* pos, const float* head, const int* state, const int* n_agents, const int* first_new, const int* type,
                       const float* shape, int S, int A_cap, int T, int c, const float* end_pose, int token_size, const float* records,
                       const unsigned char* phase, int n_phase, int K, int t, int copies, float setback, float align, const int* types,
                       const uint32_t* mask_bits, int mask_n_sets, const int* mask_row, const int* mask_type, uint32_t* out_bits,
                       int* out_count, float* out_info, void* stream);
int infgen_token_mask_signal(int handle, uint32_t* signal_bits, const int* identity_row, const float* shape, const float* end_pose,
                             const float* records, const unsigned char* phase, int n_phase, int K, int copies, float setback,
                             float align, const int* types, int* count, float* info);
int infgen_token_mask_signal_get(int handle, void* out, int capacity);

/* step scores: STEP SCORES, what a branching loop branches on - per scene slot and decode step the overlap, off-road and comfort terms
 * of the column the step just produced (k_step_score: one launch, no host read, no atomics).
 * Decode step t produces column c1 = 2 + t.  Row i of scene slot s is LIVE at a column when i < n_agents[s] and state[col][i] is not
 * invalid (0): "in the scene" of the collision masks, without first_new.  fp32 throughout, no fused multiply-add; world coordinates
 * enter only through differences formed directly from stored values, pos[j] - pos[i] and (anchor - pos[i]) + offset (the rules of the
 * collision and road masks above).  Per slot and step 8 floats, step_score[s][t][0..7], 32-byte aligned:
 *   0 n_live        rows live at c1.
 *   1 n_overlap     live rows whose box - the pose of c1, half extents shape[i][0] / 2, shape[i][1] / 2 - overlaps at least one other live
 *                   row's box: the separating-axis value sep < 0 of the collision masks, evaluated in row i's frame.
 *   2 min_sep       the minimum of sep over all ordered live pairs; +inf with fewer than two live rows.
 *   3 n_offroad     live rows whose type ty (0 vehicle, 1 pedestrian, 2 cyclist; others count as 0) has types[ty] != 0 and that are
 *                   OFF-ROAD: the row's box overlaps an obstacle rectangle - half extents (L / 2 + road_margin, road_margin) - of a
 *                   record of map scene s / copies (records, n_records, rec_cap and the never-used records of radius -1 as for the
 *                   road masks); with sweep = 1 also when the row is live at c1 - 1, its displacement d = pos[c1][i] - pos[c1 - 1][i]
 *                   is not zero and its PATH RECTANGLE - centre the midpoint of the two positions, heading that of d, half extents
 *                   (|d| / 2, the row's half width) - overlaps one.  No straddle exemption: a row sitting on an edge is off-road.
 *                   Without a record table (records NULL): 0.
 *   4 max_accel     the maximum of | |p[c1] - p[c1-1]| - |p[c1-1] - p[c1-2]| | / dt^2 over the rows live at all three columns; 0 if none.
 *   5 max_yaw_rate  the maximum of |wrap(head[c1] - head[c1-1])| / dt over the rows live at both columns; 0 if none.
 *   6, 7            0, reserved.
 * and one byte per row, score_row[s][i], of the newest step only (not history, like the collision and road buffers): bit 0 live,
 * bit 1 overlap, bit 2 off-road.  Counts are exact as floats; every reduction is a count, a min or a max, so the result is bitwise
 * reproducible whatever the reduction order.
 * infgen_step_score: one launch for column c1 of scene arrays laid out like InfgenRollout's ([S][T][A_cap]; A_cap need not be a
 * multiple of 32, at most INFGEN_Q_MAX_AGENTS); slot s writes the 8 floats at out_score + s * out_stride (floats); out_row optional
 * [S][A_cap].  Columns c1 - 1 and c1 - 2 are read only where they exist (c1 >= 1, c1 >= 2).
 * Refused: c1 outside 0 .. T - 1, a margin that is negative or not finite, dt <= 0 or not finite, sweep outside {0, 1}, copies < 1 or
 * not dividing S, a missing output, shape array or type switch, an output that is not 32-byte aligned (or a stride that is no multiple
 * of 8), a record table that is not 16-byte aligned or comes without its counts.
 * infgen_token_mask_score: attaches a score configuration to a registered token mask, as infgen_token_mask_road does (a handle
 * created with mask_bits NULL and mask_n_sets 0 constrains nothing: the heads launches stay the unmasked ones): infgen_decode_step of
 * a context that names the handle launches k_step_score after infgen_integrate of step t, for column 2 + t, and writes
 * step_score [S][steps][8] at [s][t] and score_row.  infgen_rollout_run's folded tail is not taken while it is set; with it unset the
 * launches and their arguments are exactly those without it.  infgen_branch_scenes copies the parent's [steps][8] block onto the
 * child (score_row is rebuilt by the next step).  The pointers are kept, not the contents.  step_score NULL detaches.  A context with
 * scenario insertion (first_new != NULL) that names such a handle is refused: scoring such a context is left out, as branching is. */
int infgen_step_score(const float* pos, const float* head, const int* state, const int* n_agents, const int* type, const float* shape,
                      int S, int A_cap, int T, int c1, const float* records, const int* n_records, int rec_cap, int copies, int sweep,
                      float road_margin, const int* types, float dt, float* out_score, long long out_stride, unsigned char* out_row,
                      void* stream);
int infgen_token_mask_score(int handle, float* step_score, int steps, unsigned char* score_row, const float* shape, const float* records,
                            const int* n_records, int rec_cap, int copies, int sweep, float road_margin, const int* types, float dt);

/* observations: OBSERVATIONS, what a controller reads per commanded row - for each of the N rows named, in the row's own frame, the
 * row's own features, its K nearest live agents and its Km nearest map tokens (k_observe_rows: one launch, no host read, no
 * atomics; the scene is only read).  fp32 throughout, no fused multiply-add; world coordinates enter only through differences formed
 * directly from stored values, pos[j] - pos[i] and map_pos[m] - pos[i] (the rule of the blocks above).
 *   inputs   the scene arrays laid out like InfgenRollout's ([S][T][A_cap], A_cap need not be a multiple of 32, at most
 *       INFGEN_Q_MAX_AGENTS), type [S * A_cap], shape [S * A_cap][3], column c in 0 .. T - 1, dt > 0; the map map_pos [S0][M_cap][2],
 *       map_orient [S0][M_cap], map_type [S0][M_cap] (long long, as infgen_road_records_from_map takes it), n_map [S0], S0 = S / copies:
 *       scene slot s reads map scene s / copies.  obs_row: optional int32 [N] of global rows s * A_cap + i, any order, repeats
 *       allowed; NULL: row n is n, and N must be S * A_cap.  K, Km in 0 .. INFGEN_OBS_MAX_K; radius, map_radius >= 0 or +inf.
 *   live, frame   row i of slot s is LIVE at a column iff i < n_agents[s] and state[col][i] != 0 (the step scores' rule).  An
 *       obs_row entry that is out of range or not live at c gets all-zero features, indices -1 and counts 0.  With
 *       ci = cosf(head[c][i]), si = sinf(head[c][i]) a world difference (dx, dy) becomes x' = dx * ci + dy * si, y' = dy * ci - dx * si.
 *       wrap(a) = r - pi, r = fmodf(a + pi, 2 pi), + 2 pi where negative (pi, 2 pi the nearest floats): the step scores', signed.
 *       The VELOCITY of a row j live at c and, with c >= 1, at c - 1 is ((pos[c][j] - pos[c-1][j]) / dt) - difference, then
 *       division, per component -, rotated into row i's frame; it is (0, 0) when c == 0 or j is not live at c - 1.
 *   self_feat [N][INFGEN_OBS_SELF = 8]   0 live (0 / 1); 1, 2 the row's own velocity in its own frame; 3 wrap(head[c] - head[c-1]) / dt;
 *       4, 5 length, width = shape[row][0], shape[row][1]; 6 the type as a float (0 vehicle, 1 pedestrian, 2 cyclist; others count as
 *       0); 7 has-previous: 1 iff c >= 1 and the row is live at c - 1.  Entries 1 to 3 are 0 when entry 7 is.
 *   neighbours   the candidates are the rows j != i of the same slot that are live at c; d2 = fl(fl(dx * dx) + fl(dy * dy)) with
 *       dx = pos[c][j].x - pos[c][i].x and dy likewise; j is kept iff d2 <= fl(radius * radius) (+inf keeps all; a NaN d2 is never
 *       kept).  Order: ascending d2, ties by ascending j; the first K are written.
 *       nbr_feat [N][K][INFGEN_OBS_NBR = 10]: 0, 1 x', y' of (dx, dy); 2, 3 cos D = cj * ci + sj * si, sin D = sj * ci - cj * si from
 *       cosf / sinf of the two headings (no wrap, no atan2); 4, 5 j's velocity in i's frame (an absolute velocity, not a relative
 *       one); 6, 7 j's length, width; 8 j's type; 9 1.0.  nbr_index [N][K] int32 = j.  nbr_count [N] int32 = the number of
 *       candidates inside the radius: it may exceed K, so a caller sees truncation.  Unused entries: features 0, index -1.
 *   map tokens   the candidates are m < n_map[s / copies] (at most M_cap); d2 as above from map_pos[m] - pos[c][i]; kept iff
 *       d2 <= fl(map_radius * map_radius); ascending d2, ties by ascending m; the first Km are written.
 *       map_feat [N][Km][INFGEN_OBS_MAP = 6]: 0, 1 x', y'; 2, 3 cos D, sin D of map_orient[m] against the row's heading (formulas as
 *       above); 4 (float)map_type[m]; 5 1.0.  map_index [N][Km], map_count [N] as for the neighbours.
 * Every output entry has one writer and every selection is by distinct keys (d2, index): the result is bitwise reproducible.  For any
 * content of obs_row, n_agents, n_map and state nothing outside the layouts is read or written (counts are clamped to 0 .. capacity).
 * K = 0: nbr_feat and nbr_index may be NULL, and nbr_count too (no scan then; given, it is still the count).  Km = 0 likewise; the
 * four map arrays may then be NULL (map_count, where given, is 0 without them).
 * Refused: c outside 0 .. T - 1, K or Km outside 0 .. INFGEN_OBS_MAX_K, dt <= 0 or not finite, a radius that is negative or NaN,
 * copies < 1 or not dividing S, a missing output (self_feat; with K > 0 the three nbr arrays; with Km > 0 the three map outputs and
 * the four map inputs), an output that is not 16-byte aligned, A_cap beyond INFGEN_Q_MAX_AGENTS, N < 0, or N != S * A_cap without
 * obs_row. */
#define INFGEN_OBS_SELF 8
#define INFGEN_OBS_NBR 10
#define INFGEN_OBS_MAP 6
#define INFGEN_OBS_MAX_K 64
int infgen_observe_rows(const float* pos, const float* head, const int* state, const int* n_agents, const int* type, const float* shape,
                        int S, int A_cap, int T, int c, float dt, const float* map_pos, const float* map_orient,
                        const long long* map_type, const int* n_map, int M_cap, int copies, const int* obs_row, int N, int K,
                        float radius, int Km, float map_radius, float* self_feat, float* nbr_feat, int* nbr_index, int* nbr_count,
                        float* map_feat, int* map_index, int* map_count, void* stream);

/* rule-based controlled agents: IDM COMMANDS, the next target pose of rows that follow their route under the intelligent-driver
 * car-following law (k_idm_command: one launch, no host read, no atomics) - what a closed-loop session hands to infgen_command_rows
 * as a pose command.  fp32 throughout, no fused multiply-add; world coordinates enter only through the exact differences
 * p0 - pos[c][i] and pos[c][j] - pos[c][i] (and pos[c][j] - pos[c-1][j] for the speeds).
 *   column   c is the newest stored column, 1 <= c < T.  Row i of scene slot s is LIVE at a column when i < n_agents[s] and its state
 *       there is not invalid (0): the step scores' notion, without first_new.
 *   ruled   a row is RULED iff ctl_row[s][i] != 0 (a byte per row), it is live at c, its type ty (0 vehicle, 1 pedestrian, 2 cyclist;
 *       others count as 0) has types[ty] != 0, and total > 0.  The route tables - records, total of infgen_route_records and the
 *       optional v_des [S / copies][A_cap] - are read at row (s / copies, i), as by k_route_mask.  cmd_pose is NOT written for any
 *       other row (not ruled, or padding); their out_state row is eight zeros and their out_lead is -1.
 *   speed   v = |pos[c][i] - pos[c-1][i]| / dt if the row is live at c - 1, else 0: the difference first, then
 *       sqrtf(dx * dx + dy * dy) / dt.
 *   own projection   the row's live records are moved into its frame once - translate by pos[c][i], then rotate by -head[c][i]:
 *       q0 = R(p0 - pos), u = R(ux, uy) with R(x, y) = (x ci + y si, y ci - x si), ci = cosf(head), si = sinf(head) - and the origin is
 *       projected by the route masks' rule: over the live segments in order a = min(max((e - q0) . u, 0), L), f = e - q0 - a u,
 *       d2 = |f|^2, the FIRST segment of least d2.  That gives s0 = cum + a, the segment g0 and the offset vector f;
 *       e0 = f.x * n.x + f.y * n.y with n = (-u.y, u.x) of g0 is the signed lateral offset (left of the route: positive).
 *   lead search   for every j != i live at c: the centre pos[c][j] - pos[c][i], rotated into the row's frame, is projected the same
 *       way: s_j, d_j = sqrtf(d2), the segment g_j.  j is a CANDIDATE iff d_j <= lateral + 0.5f * (w_i + w_j) and s_j > s0
 *       (w = shape[.][1], len = shape[.][0]); gap_j = (s_j - s0) - 0.5f * (len_i + len_j);
 *       vl_j = max(0, (R(pos[c][j] - pos[c-1][j]) . u(g_j)) / dt) if j is live at c - 1, else 0.  The LEAD is the candidate of least
 *       gap_j, ties to the lowest j.  With stop_at_end != 0 the route's end is a standing candidate: gap = (total - s0) - 0.5f * len_i,
 *       vl = 0, index -2; it wins only if its gap is strictly less than the best agent gap.  No candidate: lead -1, gap = +inf, and
 *       the interaction term of the law is 0.
 *   law   g = max(gap, 0.1f); v0 = v_des[route row] where v_des is given and that entry is > 0, else v0_type[ty];
 *       sstar = s_min + max(0, v * headway + v * (v - vl) / (2 * sqrtf(a_max * b_comf))); r = v / v0, free = 1 - (r * r) * (r * r),
 *       q = sstar / g (0 without a lead); acc = a_max * (free - q * q), clamped to [-b_max, a_max]; v1 = max(0, v + acc * dt);
 *       s1 = min(s0 + 0.5f * (v + v1) * dt, total).
 *   target   the first live segment in order with s1 <= cum + L, or the last live one if there is none; a1 = min(max(s1 - cum, 0), L);
 *       the point of the row's frame t = (q0 + a1 * u) + (keep * e0) * n, with that segment's u and n, is rotated back by +head -
 *       (t.x ci - t.y si, t.x si + t.y ci) - and added to pos[c][i]; heading = atan2f(uy, ux) of the record's stored world direction.
 *       cmd_pose[s][i] = (x, y, heading).
 *   outputs   out_state [S * A_cap][8] (optional, 16-byte aligned) = (s0, e0, v, gap, acc, v1, s1, 1); out_lead [S * A_cap]
 *       (optional) = j, -1 or -2.  A d_j within ~1e-4 m of its threshold, two gaps or two segments' d2 that tie that closely, or an
 *       s_j that close to s0 may fall either way.
 * infgen_idm_command: one launch of k_idm_command over the S * A_cap rows; v0_type (three floats) and types (three ints) are host
 * arrays read at the call, like the route masks' types.  A session launches it in front of infgen_command_rows with ctl_row = its
 * controlled-row flags; rows scenario insertion appends are never ruled there but count as obstacles once live.
 * Refused, each with a message and no launch: a parameter that is not finite; dt, a_max, b_comf, b_max or a v0_type entry <= 0;
 * headway, s_min or lateral < 0; keep outside [0, 1]; P outside 2..32; copies < 1 or not dividing S; c < 1 or c >= T; A_cap beyond
 * INFGEN_Q_MAX_AGENTS; a missing required pointer (everything but v_des, out_state and out_lead); records or out_state that are not
 * 16-byte aligned. */
int infgen_idm_command(const float* pos, const float* head, const int* state, const int* n_agents, const int* type, const float* shape,
                       const uint8_t* ctl_row, int S, int A_cap, int T, int c, const float* records, const float* total, int P,
                       int copies, const float* v_des, float dt, const float* v0_type, float headway, float s_min, float a_max,
                       float b_comf, float b_max, float lateral, float keep, const int* types, int stop_at_end, float* cmd_pose,
                       float* out_state, int* out_lead, void* stream);

/* ---- scenario insertion (reference agent_decoder.py:1773-2105); the sub-loop is sequenced by the host ----
 *   infgen_occupancy        one-hot sum of the grid tokens of column c (:1852-1854); tokens outside [0, grid_size) mark no cell
 *   infgen_point_edges      _build_a2sa_edge / _build_map2sa_edge for one query point per scene (:760-904):
 *                           first-K agents / map tokens (ascending index) within a radius of centre_row's pose
 *   infgen_insert_decide    seed heads -> enter / type / shape / cell, occupied-cell rejection, row append (:1883-1999);
 *                           inserted[s] = 1 row appended, 0 none, -1 the scene has no free row left (A_cap reached: the
 *                           caller must re-run with more head-room - nothing is dropped silently); a scene whose cell
 *                           logits rank no cell (all NaN) stops without a row (inserted = 0, active = 0)
 *   infgen_insert_finalize  heading token + xy offset of the new row (:2060-2074), for the scenes with inserted[s] > 0 only
 *                           (0 and -1 appended no row: nothing of the scene is touched) */
int infgen_occupancy(const InfgenRollout* r, int c, float* occ, void* stream);
/* the same plus seed_agent_occ_embed of it (MLPLayer pack of infgen_amd.packing.pack_mlp_layer) -> emb [S][128], one launch */
int infgen_occupancy_embed(const InfgenRollout* r, int c, float* occ, const float* embed_pack, float* emb, void* stream);
int infgen_point_edges(const InfgenRollout* r, int c, const int* centre_row, const int* active, int exclude_centre,
                       int which /* bit0 agents, bit1 map */, float r_agent, int k_agent, float r_map, int k_map,
                       const InfgenEdgeBuf* ea, const InfgenEdgeBuf* em, void* stream);
int infgen_insert_decide(const InfgenRollout* r, int t, int force_enter, int max_new,
                         const float* lg_state, const float* lg_type, const float* shape, const float* lg_pos,
                         const float* occ, int* active, int* n_new, int* inserted, int* new_row, float* new_shape,
                         int* new_cell, void* stream);
/* the same with the stochastic cell choice of the reference (:1900-1904) made reproducible: inverse CDF over the sample_k (<= 16)
 * most probable cells with uniform[s] in [0, 1); an occupied sampled cell spends the iteration, the scene stays active (:1906-1909) */
int infgen_insert_decide_topk(const InfgenRollout* r, int t, int force_enter, int max_new,
                              const float* lg_state, const float* lg_type, const float* shape, const float* lg_pos,
                              const float* occ, int* active, int* n_new, int* inserted, int* new_row, float* new_shape,
                              int* new_cell, int sample_k, const float* uniform, void* stream);
/* the same with temperature and nucleus truncation of the cell draw (InfgenSampling above, scalars only: temperature_row is ignored;
 * NULL: infgen_insert_decide_topk) */
int infgen_insert_decide_topk_ex(const InfgenRollout* r, int t, int force_enter, int max_new,
                                 const float* lg_state, const float* lg_type, const float* shape, const float* lg_pos,
                                 const float* occ, int* active, int* n_new, int* inserted, int* new_row, float* new_shape,
                                 int* new_cell, int sample_k, const float* uniform, const InfgenSampling* sampling, void* stream);
int infgen_insert_finalize(const InfgenRollout* r, int c, float angle_interval, const int* inserted,
                           const int* new_row, const float* lg_heading, int n_heading, const float* offset,
                           float* hv_ovr, void* stream);

/* insertion rules: INSERTION RULES, the allowed cells of scenario insertion for one column (k_insert_cell_mask: one launch, one
 * workgroup per scene, no host read, no atomics, no scratch) and the decision under them (k_insert_decide<true, true>).  Where the
 * collision, road and route masks constrain the motion tokens of rows that exist, these constrain where, what and how many rows the
 * insertion sub-loop appends.  fp32 throughout, no fused multiply-add.
 *   cells   grid_xy [G][2], the tokenizer's grid in the EGO FRAME (+y forward), G <= 8192; its values are used as stored.  allowed
 *       [S][W] little-endian 32-bit words, bit g of a scene's set = cell g allowed, W = ceil(G / 32) rounded up to a multiple of 4
 *       (16-byte rows); bits at positions >= G are 0.
 *   ego frame   column c, ego row av = av_index[s] (clamped to the layout): e = pos[c][av], phi = head[c][av] - pi / 2 (pi / 2 the
 *       nearest float), cs = cosf(phi), sn = sinf(phi).  A world point p enters only through the exact difference d = p - e (per
 *       component, formed directly from stored values), rotated: R(d) = (d.x * cs + d.y * sn, d.y * cs - d.x * sn) - the inverse of
 *       the rotation infgen_insert_decide places a cell with.  A world direction (ux, uy) is rotated by the same R.  Every test below is
 *       between a cell's grid value g = (gx, gy) and such ego-frame quantities, so magnitudes stay below ~100 m wherever the scene lies.
 *   A cell is BANNED when any rule that is switched on (`rules`, the INFGEN_IM_* bits) bans it:
 *   ego_keepout (back, front, half_width)   banned iff -back <= gy <= front and |gx| <= half_width: comparisons of stored grid
 *       values, exact.
 *   clearance   for every row j IN THE SCENE at column c (j < n_agents[s] and state[c][j] not invalid (0): the ego row and rows
 *       appended by earlier iterations of the same step included): centre q = R(pos[c][j] - e), axis u = R(cosf(head[c][j]),
 *       sinf(head[c][j])), half extents hl = max(shape[j][0] / 2, 0), hw = max(shape[j][1] / 2, 0) - the row's own length x width.
 *       With f = g - q: lx = f.x * u.x + f.y * u.y, ly = f.y * u.x - f.x * u.y, dist = sqrtf(ox * ox + oy * oy) with
 *       ox = max(|lx| - hl, 0), oy = max(|ly| - hw, 0); banned iff dist < clearance.  A row with f.x * f.x + f.y * f.y >= rr * rr,
 *       rr = (hl + hw) + clearance, is skipped first (the circle test: it cannot change a verdict beyond rounding).
 *   edge_clearance   the road-record table of the road masks (8 floats per record; map scene s / copies, its first n_records):
 *       a record of radius < 0 is never an obstacle; otherwise midpoint m = R((anchor - e) + offset), direction u = R(cos, sin),
 *       f = g - m, al = f.x * u.x + f.y * u.y, ac = f.y * u.x - f.x * u.y, dist = sqrtf(ox * ox + ac * ac) with
 *       ox = max(|al| - half_length, 0); banned iff dist < edge_clearance.
 *   near_lane (dist, types)   the cell is banned UNLESS some map token m < n_map[s / copies] (at most M_cap) whose map_type[m] is in
 *       0..31 and has its bit set in lane_types lies within dist: q = R(map_pos[m] - e), f = g - q,
 *       f.x * f.x + f.y * f.y <= dist * dist (both sides rounded to float).
 *   zones [S0][Z][4] = (x, y, r, mode) in world coordinates, the first n_zones[s / copies] of map scene s / copies: a zone whose r is
 *       not finite or <= 0, or whose mode is neither 0 nor 1, is VOID and ignored.  q = R((x, y) - e); the cell is INSIDE iff
 *       f.x * f.x + f.y * f.y <= r * r.  mode 0: a cell inside is banned.  mode 1 (allow-only): if the scene has at least one
 *       non-void zone of mode 1, a cell that is inside none of them is banned.
 *   A distance within ~1e-4 m of its threshold may fall either way (cosf / sinf and the rounding of the rotations).
 *   static / dynamic   keep-out, edges, lanes and zones depend only on the ego pose of column c: static_pass 1 evaluates them and
 *       stores static_bits [S][W] (bit = no static rule bans the cell), static_pass 2 reads static_bits instead of evaluating them
 *       (the later iterations of a step), static_pass 0 evaluates them without storing.  The clearance rule is evaluated by every
 *       pass: allowed = static AND NOT near_agent.  The same launch writes allowed_count[s] = the population count of the scene's
 *       allowed bits and live[s] = the number of rows in the scene at column c (whatever rules are on).
 *   Left out on purpose: only the cell CENTRE is tested; the offset head moves the new row by up to 2 m per axis afterwards
 *       (infgen_insert_finalize) and the new agent's own extents are not considered - callers fold both into `clearance`.  Rows not in
 *       the scene at column c (exited, not yet entered) are no obstacles.  The reference's occupied-cell test stays as it is.
 *   the decision under rules (infgen_insert_decide_mask)   as infgen_insert_decide_topk_ex, except: a banned cell is NO CANDIDATE of
 *       the rank search, greedy or sampled - with sample_k > 1 the list holds min(sample_k, allowed_count) cells and the inverse CDF
 *       re-normalises over those (the token masks' rule); a scene without an allowed cell takes the "no cell" exit (inserted = 0,
 *       active = 0, nothing else touched; there is no fallback set: a scene may simply not insert).  The occupied-cell rule applies
 *       to the chosen cell as before.  type_allowed (three host ints: vehicle, pedestrian, cyclist): the type arg-max runs over the
 *       allowed types only, first index on ties.  max_agents (optional [S], with live [S] from infgen_insert_cell_mask): enter is
 *       additionally false when live[s] >= max_agents[s]; the scene stops for the step like a lost enter logit.
 * infgen_insert_cell_mask: the operator entry; the scene arrays are laid out like infgen_collision_mask's ([S][T][A_cap], A_cap at most
 * INFGEN_Q_MAX_AGENTS), shape [S * A_cap][3]; keepout: three host floats (back, front, half_width).  Tables of rules that are off may be
 * NULL.  count_log (optional): allowed_count[s] is also written to count_log[s * count_stride].
 * Refused, each with a message and no launch: a distance that is negative or not finite; copies < 1 or not dividing S; G outside
 * 1..8192; words != W; c outside 0 .. T - 1; A_cap beyond INFGEN_Q_MAX_AGENTS; static_pass outside 0..2; a missing table of a rule
 * that is on (shape, records / n_records, map_pos / map_type / n_map, zones / n_zones, static_bits for pass 1 and 2); a missing
 * output; a bit table, record table or zone table that is not 16-byte aligned.  infgen_insert_decide_mask refuses type_allowed all
 * zero, max_agents without live, a missing or misaligned allowed table and words < ceil(grid_size / 32). */
enum { INFGEN_IM_KEEPOUT = 1, INFGEN_IM_CLEARANCE = 2, INFGEN_IM_EDGES = 4, INFGEN_IM_LANES = 8, INFGEN_IM_ZONES = 16 };
int infgen_insert_cell_mask(const float* pos, const float* head, const int* state, const int* n_agents, const int* av_index,
                            const float* shape, int S, int A_cap, int T, int c, const float* grid_xy, int G, int rules,
                            const float* keepout, float clearance, float edge_clearance, float lane_dist, unsigned lane_types,
                            const float* records, const int* n_records, int rec_cap, const float* map_pos,
                            const long long* map_type, const int* n_map, int M_cap, const float* zones, const int* n_zones, int Z,
                            int copies, int static_pass, uint32_t* static_bits, uint32_t* allowed, int words, int* allowed_count,
                            int* live, int* count_log, long long count_stride, void* stream);
int infgen_insert_decide_mask(const InfgenRollout* r, int t, int force_enter, int max_new,
                              const float* lg_state, const float* lg_type, const float* shape, const float* lg_pos,
                              const float* occ, int* active, int* n_new, int* inserted, int* new_row, float* new_shape,
                              int* new_cell, int sample_k, const float* uniform, const InfgenSampling* sampling,
                              const uint32_t* allowed, int words, const int* type_allowed, const int* max_agents, const int* live,
                              void* stream);

/* ---- the insertion sub-loop of one decode step, sequenced in the library (reference agent_decoder.py:1773-2105) ----
 * One iteration = infgen_insert_seed (occupancy + its embedding, edges into the seed node, the nine seed sublayers with the
 * previous iteration's new rows riding along edgelessly, the seed heads, the decision) -> the caller reads the per-scene
 * decisions (host_dec, pinned memory, valid once the stream reached this point) -> if any scene inserted,
 * infgen_insert_heading (categorical embedding and raw feature of the new rows, their 10 m neighbourhood through motion layers
 * 0..2, heading token + offset, final raw feature).  ~60 launches per iteration behind two calls; no host synchronisation inside.
 * All arrays are caller-allocated device memory (sizes in comments; S scenes, rows = S * A_cap, G grid cells). */
typedef struct InfgenInsertion {
  /* weights */
  const float* attn_occ2sa[3]; const float* attn_pt2sa[3]; const float* attn_a2sa[3];
  const float* four_a2sa; const float* four_pt2sa;
  const float* head_state; const float* head_type; const float* head_shape; const float* head_pos; const float* head_heading;
  const float* head_offset; const float* occ_embed; const float* shape_emb; const float* type_a_emb; const float* f_seed;
  /* per-step caches */
  float* occ; float* occ_emb;                 /* [S][G], [S][128] */
  float* Kocc[3]; float* Vocc[3];             /* [S][128] */
  const float* mapK[3]; const float* mapV[3]; /* [S * M_cap][128]: K / V of the map tokens for the pt2sa layers */
  float* Ksa[3]; float* Vsa[3]; float* Kh[3]; float* Vh[3];   /* [rows][128] */
  float* Xc;                                  /* [rows][128] */
  float* zero_agg; float* zero_z; float* zero_sig;            /* [rows][128], [rows][8][128], [rows][8]: stay zero */
  /* seed / new-row work arrays, 2 S rows each (rows [S, 2 S): the riders, one slot per scene) */
  float* XS; float* QS; float* US; float* AGGS; float* ZS; float* SIGS; float* KN; float* VN;
  InfgenEdgeBuf ea_s, em_s, ea_h, em_h;       /* off / cnt: [S] */
  const int* occ_off; const int* occ_cnt; const int* occ_src;   /* the one occupancy edge of every seed row */
  int* active; int* n_new; int* inserted; int* new_row; int* new_cell; int* new_local; float* new_shape;   /* [S] (new_shape [S][3]) */
  int* prev_row; int* prev_mask;              /* [S]: rows the previous iteration appended (seed-chain riders) */
  int* pend_row; int* pend_mask;              /* [S]: rows of the last heading stage (heading-chain riders) */
  float* hv_ovr; float* shape_all;            /* [S][2], [rows][3] */
  float* hid; float* lg_state; float* lg_type; float* shape; float* lg_pos; float* lg_heading; float* offset;
                                              /* [6][S][128], [S][2], [S][3], [S][3], [S][G], [S][n_heading], [S][2] */
  float* t1; float* t2; float* shp;           /* [S][128] each */
  int* host_dec;                              /* PINNED HOST memory [3][S]: inserted, new_row, active */
  float r_seed, r_a2sa, r_pl2sa, angle_interval;
  int n_heading, force_enter, insert_k, max_new;
  float insert_temperature, insert_top_p;     /* the cell draw's temperature / nucleus mass (InfgenSampling: 0 = unset = 1; insert_k > 1) */
  /* the ablated insertion heads (0 / NULL = the full-token model).  no_grid_token: no occupancy embedding, no occ2sa layers (the seed
   * chain is pt2sa -> a2sa x 3), head_pos_xy (seed_pos_rel_xy_predict_head, MLPLayer 128 -> 2) replaces head_pos / head_offset: the new
   * row sits at tanh(xy) * r_seed + ego pos (world frame), its grid cell is -1, insert_k is ignored.  no_head_token:
   * head_heading_theta (seed_heading_rel_theta_predict_head, 128 -> 1) replaces head_heading: heading tanh(theta) * pi + ego heading,
   * not wrapped (agent_decoder.py:1910-1912, :2060-2074) */
  const float* head_pos_xy; const float* head_heading_theta;
  int no_grid_token; int no_head_token;
} InfgenInsertion;
/* it: iteration of the step (0: map edges of the seed are built and the agents' edgeless chains are computed); riders != 0: the
 * previous iteration appended rows (prev_row / prev_mask); uniform: [S] for the cell draw when insert_k > 1 */
int infgen_insert_seed(const InfgenRollout* r, const InfgenInsertion* I, int t, int it, int riders, const float* uniform, void* stream);
/* infgen_insert_seed under insertion rules ("INSERTION RULES" above): the same launches, plus k_insert_cell_mask for the step's column
 * in front of the decision - static_pass 1 when it == 0, 2 afterwards - and the masked decision, which also writes an appended row's
 * shape to box_shape, so that the next iteration's clearance test sees its box.  The rule arguments are infgen_insert_cell_mask's
 * (keepout: three host floats, may be NULL with the rule off; the map arrays are the context's map_pos / n_map, map scene
 * s / copies, plus map_type), type_allowed / max_agents infgen_insert_decide_mask's.  box_shape [S * A_cap][3]: the caller fills the
 * rows that exist.  count_log (optional) [S][log_steps]: the iteration-0 allowed count of step t at [s][t].  Nothing is kept
 * between calls: zones / n_zones may be rewritten between two steps.  InfgenInsertion.max_new is the rules' per_step and must be
 * in 1..10; a block with no_grid_token is refused (there is no cell to mask).  infgen_insert_seed itself is unchanged. */
int infgen_insert_seed_rules(const InfgenRollout* r, const InfgenInsertion* I, int t, int it, int riders, const float* uniform,
                             int rules, const float* keepout, float clearance, float edge_clearance, float lane_dist,
                             unsigned lane_types, const float* records, const int* n_records, int rec_cap,
                             const long long* map_type, const float* zones, const int* n_zones, int Z, int copies,
                             const int* type_allowed, const int* max_agents, float* box_shape, uint32_t* static_bits,
                             uint32_t* allowed, int words, int* allowed_count, int* live, int* count_log, int log_steps,
                             void* stream);
/* h_ready == 0: the agents' edgeless chain through motion layers 0..2 is computed first; riders != 0: pend_row / pend_mask ride.
 * Must not be entered once a scene reported inserted[s] = -1 (host_dec): k_insert_cat and k_insert_finalize skip such a scene, but
 * the point edges, the raw feature rows and the rider masks of this stage take any non-zero inserted[s] as "a row was appended" and
 * would use the stale new_row[s].  The caller stops on -1 and re-runs with more head-room (infgen_amd/engine.py does). */
int infgen_insert_heading(const InfgenRollout* r, const InfgenInsertion* I, int t, int h_ready, int riders, void* stream);

/* ---- edge sets of the teacher-forced forward (reference agent_decoder.py:1104-1603) ----
 * infgen_radius_edges: torch_cluster.radius / radius_graph (agent_decoder.py:632, :710, :780, :875; map_decoder.py:91) for a
 * list of query points, with the filters the reference applies AFTER the radius call, as a compact CSR by destination:
 *   query q: destination node q_node[q] (its off / cnt entries are written; nodes without a query keep what the caller put
 *   there), pose p_pos / p_head / p_inv at index q_pt[q], candidates = indices [q_c0[q], q_c1[q]) of the candidate arrays in
 *   ascending order; the first K with d^2 < radius^2 are "found", of those the ones with index != q_self[q] (optional),
 *   c_ok[index] != 0 (optional) and pair_ok[q_pair_off[q] + index - q_c0[q]] != 0 (optional, q_pair_off < 0: no pair filter)
 *   become edges with src = c_src[index] (optional, else the index) and
 *   raw = (|d|, angle(heading vector of the query, d), wrap(c_head - p_head), index_diff ? index - q_pt[q] : 0),
 *   d = candidate - query; gap_rule 1: the invalid / gap overrides of :595-601 on both components, 2: :722-723 (query
 *   invalid), 0: none.  e->off entries get e_base added (several sets in one buffer); *e->total must be zeroed by the caller
 *   and is the number of edges afterwards (> e->cap: overflow, rows that did not fit have cnt = 0).
 * infgen_motion_features: (|motion vector|, angle(head vector, motion vector), 0, 0) per (row, column) of agent-major
 *   [rows][T] arrays with the state rules of _build_vector_a (:426-447); gap_mask (optional): entries forced to the gap (:1327) */
typedef struct InfgenRadiusEdges {
  int n_q; int _pad0;
  const int* q_node; const int* q_pt; const int* q_c0; const int* q_c1; const int* q_self; const int* q_pair_off;
  const float* p_pos; const float* p_head; const unsigned char* p_inv;
  const float* c_pos; const float* c_head; const unsigned char* c_inv; const unsigned char* c_ok; const int* c_src;
  const unsigned char* pair_ok;
  float radius; int K; int gap_rule; int index_diff;
  int e_base; int _pad1;
} InfgenRadiusEdges;
int infgen_radius_edges(const InfgenRadiusEdges* a, const InfgenEdgeBuf* e, void* stream);
int infgen_motion_features(const float* pos, const float* head, const int* state, const unsigned char* gap_mask, int rows, int T,
                           float* out, void* stream);

/* ---- agent tokenisation on the device ----
 * TokenProcessor._match_agent_token (infgen/datasets/preprocess.py:552-653; cal_polygon_contour :24-54), noise off:
 * valid [A][T] bytes, pos [A][T][2], heading [A][T], shape [A][2] = (width, length); tok = last contour of every token,
 * [n_type][n_token][4][2] indexed by type[a], or per agent (type == NULL, tables tok_agent_stride floats apart).
 * Writes token_index [A][T / shift] (int32) and token_contour [A][T / shift][4][2]. */
int infgen_match_agent_tokens(const unsigned char* valid, const float* pos, const float* heading, const float* shape,
                              const int* type, const float* tok, long long tok_agent_stride, int A, int T, int shift,
                              int n_token, int* token_index, float* token_contour, void* stream);

/* TokenProcessor._tokenize_agent (infgen/datasets/preprocess.py:335-550) in three launches: heading cleaning (:310-317) and
 * extrapolation to the token grid (:319-344) IN PLACE on valid [A][T], pos [A][T][2], heading [A][T], velocity [A][T][2]
 * (the reference modifies its inputs the same way); contour matching against tok [3][n_token][4][2] by type [A]; states,
 * token position / heading, token ids -1 (invalid) / -2 (entering), validity masks, shape reset ([A][T][3], optional).
 * wl_work: [A][2] scratch.  Outputs per agent and token step (T / shift): token_index, state_idx (int32), token_contour
 * [..][4][2], token_pos [..][2], token_heading, token_valid (all 1 when predict_state), raw_token_valid (bytes). */
int infgen_tokenize_agent(unsigned char* valid, float* pos, float* heading, float* velocity, const int* type, const float* tok,
                          const float* shape_in, float* shape_out, float* wl_work, int A, int T, int shift, int current_step,
                          int n_token, int invalid_state, int valid_state, int enter_state, int exit_state, int predict_state,
                          int* token_index, float* token_contour, int* state_idx, float* token_pos, float* token_heading,
                          unsigned char* token_valid, unsigned char* raw_token_valid, void* stream);

/* InfGen._fetch_enterings (infgen/model/infgen.py:1008-1128): token_pos [A][T][2], token_heading [A][T], state_idx [A][T]
 * (int32) of B scenes whose agents are rows agent_ptr[b] .. agent_ptr[b+1] (at most max_agents <= 2048 each), av_index [B]
 * = row of the ego inside its scene; grid_xy [grid_size][2] = Attr_Tokenizer.grid.  Per agent and step: grid_token_idx
 * (-1 = invalid or beyond radius), grid_offset_xy, heading_token_idx, sort_indices (entering agents by bearing, then the
 * ego's row), inrange / bos masks (bytes), pos_xy, heading_theta.  Optional: pt_pos [M][pt_stride] (x, y first) with
 * pt_ptr [B+1] -> pt_grid_token_idx [T][M]. */
int infgen_fetch_enterings(const float* token_pos, const float* token_heading, const int* state_idx, const int* agent_ptr,
                           const int* av_index, int B, int max_agents, int T, const float* grid_xy, int grid_size,
                           float radius, float angle_interval, int enter_state, int invalid_state, int* grid_token_idx,
                           float* grid_offset_xy, int* heading_token_idx, int* sort_indices, unsigned char* inrange_mask,
                           unsigned char* bos_mask, float* pos_xy, float* heading_theta, const float* pt_pos, int pt_stride,
                           const int* pt_ptr, int M, int* pt_grid_token_idx, void* stream);

/* InfGen.match_token_map, the matching core (infgen/model/infgen.py:918-936), noise off: traj_pos [P][3][2], theta [P],
 * sample_pt [n_token][3][2] -> token_idx [P] (int32) */
int infgen_match_map_tokens(const float* traj_pos, const float* theta, const float* sample_pt, int P, int n_token,
                            int* token_idx, void* stream);

/* ---- a rollout-metric feature on the device ----
 * compute_distance_to_nearest_object (infgen/metrics/interact_features.py:19-95): every array [B][N][T] with the evaluated
 * objects in the first n_eval rows of a scene (the order the reference builds, :48-50); work = B*N*T*9 floats of scratch;
 * out [B][n_eval][T]: signed distance to the nearest other valid object (negative = overlap), 1e10 where there is none. */
int infgen_distance_to_nearest_object(const float* cx, const float* cy, const float* length, const float* width,
                                      const float* heading, const unsigned char* valid, int B, int N, int T, int n_eval,
                                      float corner_rounding_factor, float* work, float* out, void* stream);

/* compute_kinematic_features (infgen/metrics/trajectory_features.py:37-51): x, y, z (NULL = 0), heading [n][T] -> linear
 * speed, linear acceleration, yaw rate, yaw acceleration [n][T] (NaN at both ends; accel / yaw outputs may be NULL) */
int infgen_kinematic_features(const float* x, const float* y, const float* z, const float* heading, int n, int T,
                              float seconds_per_step, float* speed, float* accel, float* yaw_rate, float* yaw_accel,
                              void* stream);
/* compute_time_to_collision_with_object_in_front (infgen/metrics/interact_features.py:96-219): arrays [B][N][T] in the
 * original object order, speed from infgen_kinematic_features, eval_idx [n_eval] ascending -> out [B][n_eval][T] seconds */
int infgen_time_to_collision(const float* cx, const float* cy, const float* length, const float* width, const float* heading,
                             const float* speed, const unsigned char* valid, const int* eval_idx, int B, int N, int T,
                             int n_eval, float* out, void* stream);

/* compute_distance_to_road_edge (infgen/metrics/map_features.py:27-79; signed distance :139-349, z stretch 3): boxes
 * [B][N][T] (cz / height may be NULL = 0), eval_idx [B][n_eval] rows of the evaluated objects, road edges of all scenes
 * as padded polylines [P][L][4] = x, y, z, valid with cyclic [P] (:82-136) and poly_off [B+1] = polyline range per scene
 * -> out [B][n_eval][T], -1e10 where the box is invalid; > 0 = off road */
int infgen_distance_to_road_edge(const float* cx, const float* cy, const float* cz, const float* length, const float* width,
                                 const float* height, const float* heading, const unsigned char* valid, const int* eval_idx,
                                 int B, int N, int T, int n_eval, const float* polylines, const unsigned char* cyclic,
                                 const int* poly_off, int L, float z_stretch, float* out, void* stream);

/* Scoring of a feature under its logged distribution (infgen/metrics/compute_metrics.py:845-878 and :744-762), fused over
 * the windows the reference unfolds: values / valid [n][T] (valid NULL = all), windows of `size` steps every `step`;
 * edges [num_bins + 1] (float32 linspace of the histogram), logp [num_bins] log-probabilities of the logged distribution.
 * -> out_sum / out_cnt [n][(T - size) / step + 1]: sum of log-probabilities over the valid steps of a window, their number */
int infgen_window_log_likelihood(const float* values, const unsigned char* valid, int n, int T, int size, int step,
                                 const float* edges, const float* logp, int num_bins, float* out_sum, int* out_cnt,
                                 void* stream);

/* compute_num_placement + compute_distance_placement (infgen/metrics/placement_features.py:6-48): x, y, z (NULL = 0) and
 * state [B][N][T], av_index [B] (row of the ego, excluded) -> num_bos / num_eos [B][T], bos / eos distance [B][N][T] */
int infgen_placement_features(const float* x, const float* y, const float* z, const int* state, const int* av_index,
                              int B, int N, int T, int enter_state, int exit_state, int* num_bos, int* num_eos,
                              float* bos_distance, float* eos_distance, void* stream);

/* Scoring of a whole validation batch in one call (infgen/metrics/compute_metrics.py:891-1103 per scenario, over the rows of
 * ALL its rollouts as compute_scenario_metrics_for_bundle concatenates them).  Bundle b = scenario * n_rollout + rollout; every
 * per-object array is padded to [B][N][.] with n_rows [B] real rows per bundle (the rest is never read for a score): valid /
 * collision bytes and the six 10 Hz features with row stride ld (T steps used), the two placement distances with row stride ld2
 * and the two counts [B][.] (int64) with row stride ldn (T2 token steps used).  Windows of `size` steps every `step`, and of
 * size / shift every step / shift at the token rate; both must give the same window count W.  table [11][136] floats, one row
 * per field in the order linear_speed, linear_acceleration, angular_speed, angular_acceleration,
 * distance_to_nearest_object, collision_indication, time_to_collision, num_placement, num_removement, distance_placement,
 * distance_removement: num_bins (<= 64), min_val, max_val, metametric_weight, edges[65], logp[64], 3 unused.
 * -> scalars [n_scenario][13] (the 11 likelihoods, metametric, simulated_collision_rate), lng [n_scenario][12][W] (the 11
 * per-window likelihoods - the counts': rollout 0's -, metametric), long_rollout [B][2][W] (num_placement / num_removement per
 * rollout), counters [3] (scenarios, scenarios with a placement score, with a removement score).  Fixed summation order. */
int infgen_bundle_scores(const unsigned char* valid, const unsigned char* collision, const float* linear_speed,
                         const float* linear_acceleration, const float* angular_speed, const float* angular_acceleration,
                         const float* distance_to_nearest_object, const float* time_to_collision,
                         const float* distance_placement, const float* distance_removement, const long long* num_placement,
                         const long long* num_removement, const int* n_rows, const float* table, int n_scenario, int n_rollout,
                         int N, int T, int ld, int T2, int ld2, int ldn, int size, int step, int shift, float* scalars,
                         float* lng, float* long_rollout, int* counters, void* stream);

/* Padded row layouts (insertion on: A_cap = agents + head-room rows per scene).  infgen_active_row_groups lists, in
 * ascending order, the 16-row groups of the [S][A_cap] layout with a row below n_agents[s] + margin (groups: capacity
 * ceil(S * A_cap / 16), n_groups: 1 int, both on the device); infgen_set_row_groups makes every split-kernel launch of the
 * attention node kernels over exactly `rows` rows visit only those groups (NULL switches it off).  Rows outside the list
 * keep their previous contents. */
int infgen_active_row_groups(const int* n_agents, int S, int A_cap, int margin, int* groups, int* n_groups, void* stream);
int infgen_set_row_groups(const int* groups, const int* n_groups, int rows);
/* the same bound for the edge kernel of those launches: n_agents [S], A_cap and the margin given to infgen_active_row_groups */
int infgen_set_row_limits(const int* n_agents, int A_cap, int margin);

/* Arithmetic of the split GEMM kernels: 3 (default) = fp16 three-term split, fp32 accuracy.  Reduced precision, for BASELINE
 * config C5 (the reference's optional bf16 trainer precision), outside the 1e-3 parity bar:
 *   1 = the hi x hi term only: fp16 operands (11 significant bits), fp32 accumulation;
 *   2 = bf16 operands: every activation operand is rounded to nearest even at 8 significant bits before it enters the matrix pipe
 *       (k_*_b16 kernels), fp32 accumulation; takes packs whose fp16 planes hold bf16-rounded weights (infgen_amd.packing.
 *       operand_bits(8) / PackedWeights(operand_bits=8)) - with default packs the weights keep 11 bits, which the library cannot
 *       see: the Python engine refuses the mismatch.
 * The edge kernels' two small GEMMs (u = q W'kr, W'vr z) stay three-term in every mode; their weights come from the same packs. */
int infgen_set_gemm_terms(int terms);

/* ---- optional profiling (bench.py roofline leg; process-global, off by default) ----
 * HIP events are recorded on the launch stream around every launch of the kernels selected by
 * `mask` (bit = INFGEN_KID_*).  infgen_prof_collect synchronises the device, returns the summed
 * duration (ms), launch count and algorithmic multiply-accumulates per kernel id and 16 device-side counters, then clears
 * the event log.  counters[n] (n < 8): rows processed by the Fourier kernel with n input dims; counters[8 + k]: edges
 * built by infgen_build_edges (k = 0 temporal, 1 map, 2 agent set; counted when INFGEN_KID_EDGE_ATTN or
 * INFGEN_KID_BUILD_EDGES is selected) - each is consumed by one edge-attention launch per layer. */
enum {
  INFGEN_KID_LINEAR = 0, INFGEN_KID_FOURIER, INFGEN_KID_ATTN_PRE, INFGEN_KID_EDGE_ATTN, INFGEN_KID_ATTN_POST,
  INFGEN_KID_HEADS, INFGEN_KID_BUILD_EDGES, INFGEN_KID_INTEGRATE, INFGEN_KID_RAWFEAT, INFGEN_KID_MAP_GRAPH,
  INFGEN_KID_MAP_HEAD, INFGEN_KID_COUNT
};
int infgen_prof_enable(unsigned mask, int max_launches);
int infgen_prof_collect(double* total_ms, int* calls, double* total_macs, unsigned long long* counters);
/* the same, plus the share of every kernel that was launched INSIDE a decode step (infgen_decode_step / infgen_rollout_run):
 * step_ms / step_calls [INFGEN_KID_COUNT]; the remainder is the prologue (map encoder, column-0 chain) and operator-level calls */
int infgen_prof_collect_steps(double* total_ms, int* calls, double* total_macs, unsigned long long* counters,
                              double* step_ms, int* step_calls);
/* after infgen_prof_enable: bracket only every stride-th launch of the selected kernels INSIDE decode steps (an event pair costs
 * ~5 us of launch-stream time; launches outside decode steps are all bracketed).  infgen_prof_seen: launches of every kernel since
 * infgen_prof_enable, bracketed or not - seen / seen_step [INFGEN_KID_COUNT] (either may be NULL). */
int infgen_prof_set_stride(int stride);
int infgen_prof_seen(int* seen, int* seen_step);

/* ---- ragged batch ingest (a PyG-style Batch of B graphs: rows of every graph concatenated, `ptr` offsets) ----
 * infgen_ingest_batch writes a rollout's scene buffers straight from the Batch's device tensors, the statements of the
 * reference's inference setup (infgen/modules/agent_decoder.py:1609-1719: filter rows invalid at column hc - 1, pad, zero the
 * future, masks) per agent-side scene s < S of graph src_graph[s].  Graph g's copies are adjacent (copies per graph); the map
 * side is written once per graph, at map scene s / copies.  Every element of every destination is written (padding included):
 * the result equals the host-side setup bit for bit.  One workgroup per (scene, part); no atomics.
 * Inputs (rows N = agent_ptr[B], tokens P_tok = pt_ptr[B]; all contiguous):
 *   agent_ptr / pt_ptr [B + 1], av_index [B] (global rows), src_graph [S];
 *   state_idx, token_idx, grid_token_idx int64 [N][T0]; token_pos f32 [N][T0][2]; token_heading f32 [N][T0];
 *   raw_valid u8 [N][T0]; valid_mask u8 [N][P]; shape f32 [N][P][3]; position f32 [N][P][pos_dim]; heading f32 [N][P];
 *   type u8 [N]; id int64 [N]; pt_position f32 [P_tok][pt_pos_dim]; pt_orientation f32, pt_token_idx int64, pt_type u8,
 *   pt_pl_type u8 [P_tok]; pt_polygon int64 [P_tok] (edge_index[1] of pt_token -> map_polygon, global); light_type u8 [n_polygons].
 * Outputs: the [S][T][A_cap] / [S][A_cap] / [S0][M_cap] rollout arrays (S0 = S / copies), the epilogue inputs
 * ([S][A_cap][...]: htok, hst, p0, h0, shp, gt [S][A_cap][P - H][2], val [S][A_cap][T], ids - fresh ids max + 1 + k on the rows
 * past the kept ones) and counts [S][3]: kept rows, ego row after filtering, rows removed before the ego.
 * The caller checks the offsets (rows per graph <= A_cap <= INFGEN_Q_MAX_AGENTS, tokens <= M_cap, every ego inside its graph,
 * hc <= T0 <= T) before the call: the offsets live on the device, the entry re-checks only the scalar geometry.  A graph that
 * breaks the row bound is not written out of bounds - its scene keeps its first min(A_cap, INFGEN_Q_MAX_AGENTS) kept rows -
 * but its results are then wrong, as are those of a graph with more tokens than M_cap (its first M_cap are kept).  Offsets past
 * the arrays' rows, or src_graph entries >= B, read past the inputs. */
typedef struct InfgenBatchIngest {
  int S, copies, A_cap, M_cap, T, T0, P, hc, H, motion_cols, pos_dim, pt_pos_dim, n_polygons, _pad0;
  const long long* agent_ptr; const long long* pt_ptr; const long long* av_index; const int* src_graph;
  const long long* state_idx; const long long* token_idx; const long long* grid_token_idx;
  const float* token_pos; const float* token_heading; const unsigned char* raw_valid;
  const unsigned char* valid_mask; const float* shape; const float* position; const float* heading;
  const unsigned char* type; const long long* id;
  const float* pt_position; const float* pt_orientation; const long long* pt_token_idx; const unsigned char* pt_type;
  const unsigned char* pt_pl_type; const long long* pt_polygon; const unsigned char* light_type;
  /* destinations */
  float* pos; float* head; int* state; int* token; int* gridtok; unsigned char* tmask; unsigned char* imask;
  unsigned char* catflag; int* atype; int* bos; float* shape10; int* n_agents; int* av;
  int* n_map; float* map_pos; float* map_orient; long long* map_tok; long long* map_type; long long* map_pl; long long* map_light;
  long long* htok; long long* hst; float* p0; float* h0; float* shp; float* gt; unsigned char* val; long long* ids;
  int* counts;
  /* log replay (all optional; replay_row == NULL: nothing of it is read or written).  replay_in u8 [N]: 1 = the row follows
   * its plan.  The plan is the logged future - columns hc .. T0 - 1 of token_idx / state_idx / token_pos / token_heading - or,
   * where a plan_* array is given (same shapes), that array.  Written in the rollout's layout for InfgenRollout.teacher_* /
   * replay_row: teacher_token / teacher_state int [S][T][A_cap], teacher_pos f32 [S][T][A_cap][2], teacher_head f32 [S][T][A_cap]
   * (teacher_pos / teacher_head may be NULL: a plan of tokens and states only), replay_row u8 [S][A_cap] - the flag of every
   * row the filter keeps, for every copy of its graph; -1 / 0 everywhere else. */
  const unsigned char* replay_in;
  const long long* plan_token; const long long* plan_state; const float* plan_pos; const float* plan_head;
  int* teacher_token; int* teacher_state; float* teacher_pos; float* teacher_head; unsigned char* replay_row;
} InfgenBatchIngest;
int infgen_ingest_batch(const InfgenBatchIngest* a, void* stream);

/* Ragged row pack: for every key k < n_keys (<= 32) and scene i < n_scenes (scene s = scene0 + i * scene_step) copy the first
 * counts[k][s * count_stride[k]] rows of src[k] + s * src_stride[k] (bytes; rows of row_bytes[k] bytes, contiguous) to dst[k] at
 * row offset sum_{i' < i} counts of scene i' (the exclusive scan runs in the kernel).  The arrays describing the keys are HOST
 * arrays; src / dst / counts are device pointers.  16-byte copies where the addresses and the byte count allow. */
int infgen_pack_rows(int n_keys, const void* const* src, const long long* src_stride, const int* row_bytes,
                     const int* const* counts, const int* count_stride, void* const* dst, int n_scenes, int scene0, int scene_step,
                     void* stream);

/* ---- validation-step metrics and the open-loop loss (infgen/utils/metrics.py, infgen/model/infgen.py:644-655) ----
 * Each entry ADDS into a caller-owned device accumulator of 8-byte slots (zeroed by the caller before the first update): integer
 * counters are int64, floating sums float64, reduced in a fixed order without float atomics (bitwise reproducible).  Index arrays
 * are int32 (..64 == 0) or int64 (..64 != 0), masks are bytes (torch.bool / uint8); row strides are in elements.  `scratch`:
 * INFGEN_VM_SCRATCH_DOUBLES doubles the float entries use for the workgroups' partial sums (one per metric object / stream). */
#define INFGEN_VM_SCRATCH_DOUBLES 3072
#define INFGEN_GRID_OVERLAP_MAX_CELLS 16384

/* StateAccuracy.update and NumInsertAccuracy.update (infgen/utils/metrics.py:499-543, :632-676; the caller's use is
 * infgen/model/infgen.py:236-237 and :765): state_idx [N][T]; valid_mask [N][T] or NULL (part 1 only).
 * acc [4] += valid, valid_count, invalid, invalid_count */
int infgen_state_accuracy(const void* state_idx, int idx64, int N, int T, long long ld, const unsigned char* valid_mask,
                          long long ld_mask, int invalid_state, int valid_state, int enter_state, int exit_state, long long* acc,
                          void* stream);
/* GridOverlapRate.update (infgen/utils/metrics.py:574-591; infgen/model/infgen.py:241-242) for n_group row ranges ptr[g]..ptr[g+1]
 * (ptr NULL: one group of all N rows, the reference's behaviour): state_token / grid_index [N][>= num_step], -1 = out of range,
 * cells in [0, grid_size), grid_size <= INFGEN_GRID_OVERLAP_MAX_CELLS.
 * acc [4][num_step] += num_overlap_t, num_insert_agent_t, num_total_agent_t, num_exceed_seed_t (once per group) */
int infgen_grid_overlap(const void* state_token, int state64, long long ld_state, const void* grid_index, int grid64,
                        long long ld_grid, int N, int num_step, const long long* ptr, int n_group, int grid_size, int enter_state,
                        int seed_size, long long* acc, void* stream);
/* minADE.update (infgen/utils/metrics.py:441-464) and minFDE.update (:378-387) in one pass: pred / target [N][T][2], valid [N][T].
 * ade_acc / fde_acc [2] = (float64 sum, int64 count), either may be NULL */
int infgen_traj_error(const float* pred, const float* target, const unsigned char* valid, int N, int T, void* ade_acc,
                      void* fde_acc, double* scratch, void* stream);
/* pred[mask] + torch.nn.CrossEntropyLoss(weight, label_smoothing) of infgen/model/infgen.py:147-152, :644, :655 without the gather:
 * logits [R][C] row stride ld, target [R], mask [R], weight [C] or NULL.  acc [3] (float64) += S1 = sum w_y (-log p_y),
 * S2 = sum_i sum_c w_c (-log p_ic) (only when label_smoothing != 0), S3 = sum w_y over the selected rows; the mean loss is
 * ((1 - eps) S1 + eps / C S2) / S3.  Masked-out rows are not read; a target outside [0, C) is skipped. */
int infgen_masked_cross_entropy(const float* logits, long long ld, const void* target, int target64, const unsigned char* mask,
                                const float* weight, int R, int C, float label_smoothing, double* acc, double* scratch,
                                void* stream);
/* TokenCls.update (infgen/utils/metrics.py:326-333; infgen/model/infgen.py:725, :761): pred [R][>= n_guess] row stride ld_pred,
 * target [R], mask [R].  acc [2] (int64) += hits under the mask, mask count */
int infgen_token_cls(const void* pred, int pred64, long long ld_pred, int n_guess, const void* target, int target64,
                     const unsigned char* mask, int R, long long* acc, void* stream);
/* AverageMeter.update (infgen/utils/metrics.py:477-479): acc [2] = (float64 sum += sum of val [n], int64 count += n) */
int infgen_average_meter(const float* val, long long n, void* acc, double* scratch, void* stream);
/* minMultiADE.update (infgen/utils/metrics.py:403-424) and minMultiFDE.update (:349-361) in one pass, valid_filter (:115-140) and
 * topk (:43-76, the plain form: no joint / ptr variants) included: pred [N][M][T][2], target [N][T][2], prob [N][M] or NULL,
 * valid [N][T]; M <= 64.  A row takes part if any step is valid (keep_invalid_final_step != 0) or if its last step is (== 0).
 * The guesses are all M modes when max_guesses >= M, else the max_guesses largest prob - PINNED: ties go to the lower index, where
 * torch.topk leaves them open - or, without prob, the first max_guesses modes.  last = the last valid step.  FDE = the minimum
 * over the guesses of the distance at `last`.  ADE, ade_criterion 0 ('FDE'): the masked mean distance of the guess with the
 * smallest FDE - PINNED: the first minimum in guess order; 1 ('ADE'): the minimum over the guesses of the masked mean.
 * ade_acc / fde_acc [2] = (float64 sum, int64 count += rows taking part), either may be NULL.  Distances and sums are float64. */
int infgen_multi_traj_error(const float* pred, const float* target, const float* prob, const unsigned char* valid, int N, int M,
                            int T, int max_guesses, int keep_invalid_final_step, int ade_criterion, void* ade_acc, void* fde_acc,
                            double* scratch, void* stream);

/* ---- modes: K representative futures per agent from N candidate trajectories (the copies of a scene) ----
 * batch_nms (infgen/utils/metrics.py:198-256, mode 'static') and new_batch_nms (:143-195) in one launch: one wave per row, one
 * candidate per lane, 1 <= N <= 64, 1 <= K <= min(N, 16); anything else is refused.
 * Layout: row b < B is row r = b % rows_per_group of group g = b / rows_per_group; step t of its candidate j starts at
 *   traj + g group_stride + r row_stride + j cand_stride + t step_stride   (strides in elements, step_stride >= F)
 * and holds F floats, the first two (x, y).  A contiguous [B][N][T][F] is (rows_per_group 1, group_stride N T F, row_stride 0,
 * cand_stride T F, step_stride F); a rollout's pred_traj [S0][copies][A_cap][R][2] is read in place with rows_per_group A_cap,
 * group_stride copies A_cap R 2, row_stride R 2, cand_stride A_cap R 2, step_stride 2.
 * Goal: (x, y) at step t_goal.  Score: score [B][N] (score_per_group != 0: [groups][N], every row of a group takes its group's),
 * finite and >= 0 - or NULL: the density of new_batch_nms, float(count_j) / float(N) with count_j the valid candidates i, j
 * included, whose goal is within dist_thresh of j's.
 * PINNED by definition, where the reference leaves it open:
 *   order      score descending, then candidate index ascending (argsort(descending=True) leaves ties open);
 *   selection  K times: among the unselected valid candidates the largest value, value = score if the candidate is not covered
 *              and 0 if it is, ties to the earlier candidate of the order; the pick is marked selected and every candidate whose
 *              goal is within dist_thresh of the pick's - the pick included - covered.  For scores >= 0 this is the reference's
 *              point_val bookkeeping (covered -> 0, selected -> negative, K <= N);
 *   distance   fp32 sqrt(dx dx + dy dy) < dist_thresh: products and sum rounded separately, no contraction, square root and the
 *              density's division correctly rounded;
 *   validity   a candidate is valid unless cand_valid [B][N] (bytes, optional) is 0, or cand_state (optional, f32, addressed
 *              g state_group_stride + r state_row_stride + j state_cand_stride + t_goal) equals state_invalid or state_enter, or
 *              r >= row_limit[g limit_stride] (optional).  An invalid candidate is never picked, covers nothing and counts in no
 *              density; a row with fewer than K valid candidates fills the rest with index -1, score 0 and a zero trajectory.
 *              The reference has no mask: with every candidate valid the result is its result.
 * Outputs: mode_idx [B][K] the candidate index, mode_score [B][K] the pick's own score (covered or not, as the reference returns
 * it), mode_traj [B][K][T][F] (optional) the K winning trajectories, copied 16 bytes per lane where the addresses allow. */
int infgen_select_modes(const float* traj, long long group_stride, long long row_stride, long long cand_stride, long long step_stride,
                        int rows_per_group, long long B, int N, int T, int F, int t_goal, int K, float dist_thresh,
                        const float* score, int score_per_group, const unsigned char* cand_valid, const float* cand_state,
                        long long state_group_stride, long long state_row_stride, long long state_cand_stride, float state_invalid,
                        float state_enter, const int* row_limit, long long limit_stride, int* mode_idx, float* mode_score,
                        float* mode_traj, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* INFGEN_HIP_H_ */
