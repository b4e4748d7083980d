// Kernel argument blocks (plain structs, device pointers) and kernel declarations.
#pragma once
#include <type_traits>
#include "tile.cuh"
#include "layout.h"
#include "../../include/infgen_hip.h"

namespace ig {

struct LinearArgs {
  const float* X; int ldx; const int* gather;
  int rows; int K; int Kp;
  const float* Wp; int Np; const float* bias; int N;
  const float* pre_g; const float* pre_b;
  const float* post_g; const float* post_b; int relu;
  float* Y; int ldy;
};

constexpr int LINEAR_MULTI_MAX = 6;
struct LinearMultiArgs { LinearArgs d[LINEAR_MULTI_MAX]; };

struct FourierArgs {
  const float* raw;        // [E][4]
  int n;                   // continuous dims (2..4)
  const int* count_dev;    // optional device-side row count
  int e_cap;               // row count (or capacity when count_dev != null)
  const float* pack;       // FourierLayout
  const float* cat; int ldcat;   // optional [E][ldcat] categorical embedding sum
  float* out; int ldo;
  int normalize;
  unsigned long long* prof_rows;   // optional [8]: rows processed, indexed by n (profiling only)
  int out_r24;             // k_fourier_h only: 1 rows in the packed 24-bit format (R24_ROW_BYTES per row, below) instead of fp32
  // k_fourier_h only - the LAST input dim as a lookup (temporal edges: the time gap j - c is one of -1 .. -16, edge_kernels.hip):
  // dt_mode 1: dims 0 .. n - 2 are evaluated, row (int)(-raw[e][n - 1]) of dt_tab [DT_TAB_ROWS][128] is added to their sum
  //            (8 of the 4 (2 n + 1) weight quarters per tile are never staged);
  // dt_mode 2: writes that table - row e = the last dim's branch mlps[n - 1](-e) without its bias (the bias sum stays in the pack)
  const float* dt_tab; int dt_mode;
  int dbg;                 // diagnostics (INFGEN_QS_DBG; wrong results): 1 free-running waves over a static weight ring
};
constexpr int DT_TAB_ROWS = 32;
// k_fourier_h geometry (experiments: -DIG_FH_WAVES=4 -DIG_FH_RING=4 builds the two-workgroups-per-CU variant)
#ifndef IG_FH_WAVES
#define IG_FH_WAVES 8
#endif
// IG_QSU = 1: k_fourier_h and the 8-wave k_attn_h take their weights from the unit-granular stream (split.cuh: QuarterStreamU,
// one workgroup barrier per GEMM instead of one per quarter-matrix; 8 quarter buffers)
#ifndef IG_QSU
#define IG_QSU 0
#endif
// IG_FH_AP = 1 (default): k_fourier_h as two groups of four waves one phase apart (fourier_ap_body.inc: the matrix phases of
// one wave of a SIMD run under the vector phases of the other); 0: all eight waves in step, one barrier per quarter
#ifndef IG_FH_AP
#define IG_FH_AP 1
#endif
#ifndef IG_FH_RING
#define IG_FH_RING ((IG_QSU || IG_FH_AP) ? 8 : 5)
#endif
constexpr int FH_WAVES = IG_FH_WAVES;
constexpr int FH_NT = 64 * FH_WAVES;     // threads per workgroup
constexpr int FH_TILE = 16 * FH_WAVES;   // edges per workgroup tile (16 per wave)
constexpr int FH_RING = IG_FH_RING;      // quarter buffers of its weight ring
constexpr int FH_WG_PER_CU = FH_WAVES == 8 ? 1 : 2;
#ifndef IG_AH_RING4
#define IG_AH_RING4 3
#endif
#ifndef IG_AH_RING8
#define IG_AH_RING8 (IG_QSU ? 8 : 5)
#endif
struct FourierMultiArgs { FourierArgs set[4]; };      // (the fourth: the rows' x_a_emb embedding, infgen_rollout_run)

// Packed 24-bit rows of the normalised relative-position embedding (the rollout's private edge buffers; k_fourier_h writes,
// k_edge_fused reads): the upper 24 bits of every fp32 value (sign, exponent, 15 mantissa bits, round to nearest even) as two
// planes per row - 128 x 16 bit (bits 31..16) then 128 x 8 bit (bits 15..8): 384 B instead of 512.  The values are O(1)
// (affine-free LayerNorm output): relative error 2^-17, 32 x below fp16; the edge loop is bound by the bytes it gathers.
constexpr int R24_ROW_BYTES = 384;
constexpr int R24_LO_PLANE = 256;

// One edge set in CSR-by-destination form (built on the device every decode step).
struct EdgeSet {
  const int* off;          // [rows] first edge of the row
  const int* cnt;          // [rows] number of incoming edges
  const int* src;          // [E] row index into the K/V source arrays
  const float* rhat;       // [E][128] normalised relative-position embedding (nullptr: no pos emb)
};

struct AttnPreArgs {
  const float* X; int rows;          // [rows][128] layer input
  const float* pack;                 // AttnLayout
  int use_src_ln;                    // 1: LayerNorm with the *_src parameters (K/V of a bipartite source)
  float* Q;                          // [rows][128]   (scaled q), may be null
  float* U;                          // [rows][8][128] absorbed relative-position query, may be null
  float* K; float* V;                // [rows][128] each, may be null
};

struct EdgeAttnArgs {
  int rows;
  const float* Q; const float* U;
  const float* Ksrc; const float* Vsrc;    // source K/V arrays, row stride 128
  EdgeSet es;
  float* AGG;                        // [rows][128]  sum_e attn * v_src
  float* Z;                          // [rows][8][128] sum_e attn * rhat   (pos-emb layers only)
  float* SIG;                        // [rows][8]    sum_e attn
  const float* wkr;                  // unused (kept for layout stability)
  const int* n_agents; int A_cap, margin;   // optional (k_edge_attn): rows at or beyond n_agents[s] + margin of their scene are skipped
  const int* row_mask;               // optional (k_edge_attn_wide): rows with row_mask[row] == 0 are treated as edgeless
};

// k_edge_fused (edge_fused.hip): edge attention of a 16-row tile with the absorbed query and the positional aggregate kept on
// chip: q in, agg' = sum_e a_e v_src + W'_vr z + b' sigma out (what k_attn_h / k_attn_post then take with has_pos = 0)
struct EdgeFusedArgs {
  int rows;
  const float* Q;                    // [rows][128] scaled query
  const float* pack;                 // AttnLayout of the layer (AH_HDR scales, W'_kr / W'_vr quarter-matrices, AL_BVR)
  const float* Ksrc; const float* Vsrc;
  EdgeSet es;                        // rhat must be present
  float* AGG;                        // [rows][128] out
  const int* groups; const int* n_groups;   // optional: the 16-row groups to process (k_active_groups)
  int dbg;                           // timing experiments only (INFGEN_EDGE_DBG): bit 0 no edges
  int tiles_per_scene;               // > 1: XCD-aware tile order (rows of a scene are A_cap = 32 * tiles_per_scene consecutive rows)
  int kv_once;                       // 1: every K / V source row is read once (temporal ring): non-temporal loads
  int n_virtual;                     // tile slots to visit (tiles rounded up to whole XCD groups)
  unsigned* dbgbuf;                  // k_edge_fused_p only (INFGEN_EDGE_DBG bit 3): [rows][12] checksums of the hand-offs between the phases
  WarmArgs warm;                     // one-group variant only
};

// k_layers_p (layers_p.hip): every sublayer of a decode step in one launch for up to 256 16-row groups; one workgroup owns a group
constexpr int LP_MAX_LAYERS = 8;
struct LayersPArgs {
  int rows, A_cap, num_layers;
  int xcd_order;                     // 1: a scene's workgroups share an XCD (workgroups a multiple of 8 * A_cap / rows_per_wg)
  int row0;                          // first row of this launch (a batch beyond one launch's workgroup limit runs as chunks of whole scenes)
  int rows_per_wg;                   // 16, or 8 (the smallest batches: one row per wave in the edge loop, lanes j >= 8 are shadows)
  float* X;                          // [rows][128] in / out: the layer stack's input rows (raw features) -> its output
  const float* attn_t[LP_MAX_LAYERS]; const float* attn_m[LP_MAX_LAYERS]; const float* attn_a[LP_MAX_LAYERS];
  float* ringK[LP_MAX_LAYERS]; float* ringV[LP_MAX_LAYERS];      // [ring][rows][128]
  size_t slot_off;                   // floats: the current column's slot of the ring
  const float* mapK[LP_MAX_LAYERS]; const float* mapV[LP_MAX_LAYERS];
  float* Ka[2]; float* Va[2];        // agent-set K / V rows, double buffered by layer parity
  EdgeSet et, em, ea;
  int* sync;                         // [scenes] zeroed before the launch: arrivals of a scene's workgroups per layer
  unsigned spin_limit;               // 0: wait at the scene counters without limit (cooperative launch: residency is guaranteed);
                                     // n: trap after n polls (diagnostics, and launches captured into a HIP graph)
  unsigned long long* trace;         // diagnostics (INFGEN_LP_TRACE=1): [1024][2] (stamp id, s_memtime) of workgroup 0
};

struct AttnPostArgs {
  float* X; int rows;                // in/out residual stream
  const float* pack;
  const float* AGG; const float* Z; const float* SIG;
  int has_pos;
  // optional fused prologue of the NEXT layer on the freshly written rows (k_attn_pre's work)
  const float* next_pack;            // null: none
  float* nQ; float* nU; float* nK; float* nV;
};

// k_attn_h (attn_h.hip): the node side of one AttentionLayer on the fp16 matrix pipe - any of
//   post:  everything after the edge aggregation of layer `pack` (k_attn_post's work), in place on X
//   pre:   LayerNorm + q / u / k / v projections of layer `next_pack` on the (updated) rows (k_attn_pre's work)
struct AttnHArgs {
  float* X; int rows;
  const float* pack;                 // layer whose post part runs (null: none)
  const float* AGG; const float* Z; const float* SIG;
  int has_pos;
  const float* next_pack;            // layer whose pre part runs (null: none)
  int next_src_ln;                   // 1: LayerNorm with the *_src parameters (K/V of a bipartite source)
  float* nQ; float* nU; float* nK; float* nV;
  const int* groups; const int* n_groups;   // optional: the 16-row groups to process (device list + count), see k_active_groups
  int dbg;                           // diagnostics (INFGEN_QS_DBG; wrong results): 1 free-running waves over a static weight ring
  WarmArgs warm;                     // k_attn_hs only
};

struct ActiveGroupsArgs { const int* n_agents; int S, A_cap, margin; int* groups; int* n_groups; };

// metric_kernels.hip: compute_distance_to_nearest_object; all arrays [B][N][T], evaluated objects first
struct NearestArgs {
  const float* cx; const float* cy; const float* length; const float* width; const float* heading;
  const unsigned char* valid;
  int B, N, T, n_eval;
  float rounding;                    // corner_rounding_factor (0.7)
  float* work;                       // [B][N][T][9] scratch: shrunk corners + shrink radius
  float* out;                        // [B][n_eval][T]
};

struct KinematicArgs {               // compute_kinematic_features; x, y, z (may be null), heading: [n][T]
  const float* x; const float* y; const float* z; const float* heading;
  int n, T; float dt;
  float* speed; float* accel; float* yaw_rate; float* yaw_accel;      // [n][T]; all but speed may be null
};
struct TtcArgs {                     // compute_time_to_collision_with_object_in_front; arrays [B][N][T] in ORIGINAL object order
  const float* cx; const float* cy; const float* length; const float* width; const float* heading; const float* speed;
  const unsigned char* valid;
  const int* eval_idx;               // [n_eval] evaluated objects, ascending
  int B, N, T, n_eval;
  float* out;                        // [B][n_eval][T]
};

struct TokenizeArgs {                // _tokenize_agent bookkeeping (k_tokenize_prep / k_tokenize_state)
  unsigned char* valid; float* pos; float* heading; float* velocity;       // [A][T], [A][T][2], [A][T], [A][T][2] in/out
  const int* type; float* wl;                                              // [A], [A][2] out (width, length)
  const float* shape_in; float* shape_out;                                 // [A][T][3] (may be null)
  int A, T, shift, current_step;
  int invalid_state, valid_state, enter_state, exit_state, predict_state;
  int* token_index; const float* token_contour;                            // [A][T/shift] in/out, [A][T/shift][4][2]
  int* state_idx; float* token_pos; float* token_heading;                  // [A][T/shift](,2)
  unsigned char* token_valid; unsigned char* raw_token_valid;              // [A][T/shift]
};

struct EnteringsArgs {               // _fetch_enterings (k_fetch_enterings / k_pt_grid_cells)
  const float* token_pos; const float* token_heading; const int* state_idx;    // [A][T][2], [A][T], [A][T]
  const int* agent_ptr; const int* av_index;                                   // [B+1], [B] (row inside the scene)
  int B, T; const float* grid_xy; int grid_size;
  float radius, angle_interval; int enter_state, invalid_state;
  int* grid_token_idx; float* grid_offset_xy; int* heading_token_idx; int* sort_indices;
  unsigned char* inrange_mask; unsigned char* bos_mask; float* pos_xy; float* heading_theta;
  const float* pt_pos; int pt_stride; const int* pt_ptr; int M; int* pt_grid_token_idx;   // [M][pt_stride], [B+1], [T][M]
};

struct RoadEdgeArgs {                // compute_distance_to_road_edge; boxes [B][N][T]
  const float* cx; const float* cy; const float* cz; const float* length; const float* width; const float* height;
  const float* heading; const unsigned char* valid; const int* eval_idx;     // eval_idx [B][n_eval]
  const float* poly; const unsigned char* cyclic; const int* poly_off;       // [P][L][4], [P], [B+1]
  int B, N, T, n_eval, L; float z_stretch;
  float* out;                                                                // [B][n_eval][T]
};

struct WindowLoglikArgs {            // k_window_loglik
  const float* values; const unsigned char* valid;      // [n][T]; valid may be null (all)
  int n, T, size, step;
  const float* edges; const float* logp; int nb;        // [nb + 1], [nb], nb <= 64
  float* out_sum; int* out_cnt;                         // [n][(T - size) / step + 1]
};

struct PlacementArgs {               // placement_features; arrays [B][N][T]
  const float* x; const float* y; const float* z;      // z may be null
  const int* state; const int* av_index;               // [B][N][T], [B]
  int B, N, T, enter_state, exit_state;
  int* num_bos; int* num_eos;                          // [B][T]
  float* bos_distance; float* eos_distance;            // [B][N][T]
};

struct BundleScoreArgs {             // k_bundle_field / k_bundle_meta (bundle_scores.hip); bundle b = scenario * R + rollout
  const unsigned char* valid; const unsigned char* collision;          // [B][N][.] bytes, row stride ld
  const float* feat[4]; const float* dist; const float* ttc;            // [B][N][.] floats, row stride ld (T columns used)
  const float* d_place; const float* d_remove;                          // [B][N][.] row stride ld2 (T2 columns used)
  const long long* n_place; const long long* n_remove;                  // [B][.] row stride ldn (T2 columns used)
  const int* n_rows;                                                    // [B] object rows of a bundle (the rest is padding)
  const float* table;                                                   // [11][BS_TABLE_STRIDE] packed histograms
  int S, R, N, T, ld, T2, ld2, ldn, size, step, size2, step2, shift, W;   // windows: size / step at 10 Hz, size2 / step2 at the token rate
  float* scalars; float* lng; float* long_rollout; int* counters;       // [S][13], [S][12][W], [B][2][W], [3]
};
constexpr int BS_TABLE_STRIDE = 136;  // nb, lo, hi, weight, edges[65], logp[64], pad
constexpr int BS_FIELDS = 11;

// k_mlpemb_h (mlp_h.hip): MLPEmbedding with K0 = 128 j on the fp16 split
struct MlpEmbHArgs {
  const float* X; int ldx; int rows; int K0;
  const float* pack;                 // packing.pack_mlp_embedding incl. its split section
  float* Y; int ldy;
};

// k_match_tokens (token_kernels.hip): TokenProcessor._match_agent_token, one workgroup per agent
struct MatchTokensArgs {
  const unsigned char* valid;        // [A][T]
  const float* pos;                  // [A][T][2]
  const float* heading;              // [A][T]
  const float* shape;                // [A][2] = (width, length)
  const int* type;                   // [A] index into tok (null: per-agent tables, tok_agent_stride floats apart)
  const float* tok;                  // [3 or A][n_token][4][2] last contour of every token
  long long tok_agent_stride;
  int A, T, shift, n_token;
  int* token_index;                  // [A][T / shift]
  float* token_contour;              // [A][T / shift][4][2]
};

// k_command_rows (token_kernels.hip): a closed-loop session's commands of one decode step -> column c + 1 of the plan arrays the
// flagged rows follow (IntegrateArgs.teacher_*); one workgroup per (scene, row), the ones without a flag leave at once
struct CommandRowsArgs {
  int S, A_cap, T, c;                // writes column c + 1 (k_integrate's c / n)
  int kind;                          // 0: token ids, 1: target poses matched against the vocabulary
  int token_size;
  const int* n_agents;               // [S]
  const unsigned char* replay_row;   // [S][A_cap]
  const int* state;                  // [S][T][A_cap] stored states (column c is read)
  const float* pos; const float* head;   // [S][T][A_cap](x2) stored poses (column c is read)
  const int* type;                   // [S][A_cap]
  const float* vocab;                // [3][token_size][6][4][2]
  const float* shape;                // [S][A_cap][3] = (length, width, height); kind 1 only
  const int* cmd_token;              // [S][A_cap] (kind 0)
  const float* cmd_pose;             // [S][A_cap][3] = x, y, heading in the world frame (kind 1)
  const unsigned char* cmd_mask;     // optional [S][A_cap]: 0 = the row leaves the scene at this step
  int* teacher_token; int* teacher_state;      // [S][T][A_cap]
  float* teacher_pos; float* teacher_head;     // optional: the commanded pose is stored too (kind 1)
  float* cmd_cost;                   // optional [S][A_cap]: the winning cost of a pose command (0 for a token command)
};

// k_match_map_tokens (token_kernels.hip): InfGen.match_token_map, one wave per polyline piece
struct MatchMapArgs {
  const float* traj_pos;             // [P][3][2]
  const float* theta;                // [P]
  const float* sample_pt;            // [n_token][3][2]
  int P, n_token;
  int* token_idx;                    // [P]
};

// temperature and nucleus (top-p) truncation of the top-k samplers (topk_inverse_cdf below; InfgenSampling of include/infgen_hip.h
// after the host's checks): temperature > 0, top_p in (0, 1]; temperature_row (optional, one entry per row, >= 0) wins over the scalar,
// and an entry of 0 makes that row greedy.  The defaults (1, 1, NULL) are the plain top-k sampler bit for bit
struct SamplingCtl { float temperature; float top_p; const float* temperature_row; };
constexpr SamplingCtl SAMPLING_DEFAULT{1.0f, 1.0f, nullptr};

// per-row allowed-token sets of the motion-token heads and samplers (the token mask of include/infgen_hip.h after the host's checks):
// bits = n_sets sets of token_size / 32 little-endian words, bit c set = token c allowed.  bits == NULL: no mask (today's kernels)
struct TokenMaskCtl { const unsigned* bits; int n_sets; const int* mask_row; int mask_type[3]; const int* type; };
constexpr TokenMaskCtl TOKEN_MASK_NONE{nullptr, 0, nullptr, {-1, -1, -1}, nullptr};
// the masked instantiations of a kernel take its argument block with the mask appended; the unmasked ones keep the block - and so
// their code objects - exactly as they were
template <class A> struct Masked : A { TokenMaskCtl mask; };
template <class A, bool MK> using ArgsFor = std::conditional_t<MK, Masked<A>, A>;
constexpr int TOPK_NONE = 0x7fffffff;     // the column of a top-k slot that holds no token (fewer allowed tokens than slots)

// the row's set (its first word), NULL where the row is unconstrained: mask_row[row] >= 0 wins, else mask_type[type[row]]; an index
// beyond the table reads as unconstrained, so nothing outside bits[0 .. n_sets * words) is ever read
__device__ __forceinline__ const unsigned* token_mask_set(const TokenMaskCtl& m, int row, int words) {
  int s = m.mask_row ? m.mask_row[row] : -1;
  if (s < 0 && m.type) {
    const int ty = m.type[row];
    s = ty == 0 ? m.mask_type[0] : ty == 1 ? m.mask_type[1] : ty == 2 ? m.mask_type[2] : -1;
  }
  return (s >= 0 && s < m.n_sets) ? m.bits + (size_t)s * words : nullptr;
}

struct HeadsArgs {
  const float* X; int rows;
  const float* tok_pack;    // MLPLayer pack: P(128,128) W0, b0, ln g/b, P(128,2048) W3, b3
  const float* st_pack;     // MLPLayer pack: P(128,128) W0, b0, ln g/b, W3 [3][128] row-major, b3[3]
  int token_size;
  float* logits;            // optional [rows][token_size]
  int* next_token;          // [rows]
  int* next_state;          // [rows] raw argmax in {0,1,2}
  // k_heads only, few rows: the token_size / 128 logit chunks dealt to gridDim.y = nsplit workgroups per row tile; each merges its
  // (max, first index) into part[row] as an ordered 64-bit key (atomicMax; zeroed by the caller), k_heads_finish decodes them
  unsigned long long* part; int nsplit;
  // k_heads_h<TERMS, true> only: optional [rows], the full-softmax log-probability of next_token[row] (k_heads_h<TERMS, false> and
  // k_heads never look at it: infgen_token_logprob serves them from stored logits)
  float* token_logprob;
  // k_heads_h<TERMS, LP, KS> with KS > 0 only (top-k sampling inside the kernel, 2 <= sample_k <= KS): next_token[row] is drawn by
  // inverse CDF over the row's sample_k best logits with uniform[row] (k_sample_topk's order and arithmetic); token_logprob, when
  // given, is then the sampled token's; sample_logprob (optional [rows]) its log-probability under the re-normalised top-k
  int sample_k;
  const float* uniform;
  float* sample_logprob;
  SamplingCtl ctl;          // (KS > 0 only) temperature / top-p of the draw, read once per row next to uniform[row]
};
// (the masked instantiations k_heads_h<TERMS, LP, KS, true> and k_heads<true> take Masked<HeadsArgs>: a banned column's logit counts
// as -inf for the arg-max, the running top-k and the draw; stored logits and token_logprob stay the model's own)
constexpr int HEADS_KS = 16;      // the one sampling width k_heads_h is instantiated with (wider beams take k_sample_topk)

// the map encoder's token_predict_head (map_decoder.py:119-121) over gathered rows: logits and the 10 most probable tokens
constexpr int MAP_HEAD_N = 1024, MAP_TOPK = 10;
struct MapHeadArgs {
  const float* X; int ldx; const int* gather; int rows;
  const float* pack;        // MLPLayer pack (packing.pack_mlp_layer): P(128,128) W0, b0, ln g/b, P(128,1024) W3, b3, split section
  float* logits;            // [rows][MAP_HEAD_N]
  long long* top;           // [rows][MAP_TOPK], descending
};
__global__ void k_heads_finish(const unsigned long long* part, int rows, int* next_token);

// ---- per-scene state (column-major per scene: [S][T][A_cap]) -----------------------------------
struct SceneState {
  int S, A_cap, T, M_cap, W;        // W = temporal window (time_span / shift)
  int ring;                         // ring slots of the temporal K/V cache (> W)
  const int* n_agents;              // [S]
  const int* n_map;                 // [S]
  const int* av_index;              // [S]
  float* pos;                       // [S][T][A_cap][2]
  float* head;                      // [S][T][A_cap]
  int* state;                       // [S][T][A_cap]
  int* token;                       // [S][T][A_cap]
  int* grid;                        // [S][T][A_cap]
  unsigned char* tmask;             // [S][T][A_cap]
  unsigned char* imask;             // [S][T][A_cap]
  unsigned char* catflag;           // [S][T][A_cap] 1: own type/shape embedding, 0: seed/invalid-shape
  const int* type;                  // [S][A_cap]
  int* bos;                         // [S][A_cap] first 'enter' column (0 if none)
  const float* map_pos;             // [S][M_cap][2]
  const float* map_orient;          // [S][M_cap]
  const int* map_scene;             // optional [S]: slot of scene s in the map-side arrays (n_map, map_pos, map_orient, map K / V rows)
  // scenario insertion (optional, may be null): rows >= first_new[s] inserted in the current step carry
  // the newest row's head vector during the motion stage (reference agent_decoder.py:2083, SURVEY a-Q13)
  const int* first_new;             // [S]
  const float* hv_ovr;              // [S][2]
};

struct EdgeBuf {                    // device-side builder outputs for one edge type
  int* off; int* cnt; int* src; float* raw; int* total; int cap;
};

// forward_kernels.hip: torch_cluster.radius with an emit filter for a list of query points (the teacher-forced forward's
// edge sets and the map-token graph); include/infgen_hip.h: InfgenRadiusEdges has the field-by-field description
struct RadiusEdgesArgs {
  int n_q;
  const int* q_node; const int* q_pt; const int* q_c0; const int* q_c1; const int* q_self; const int* q_pair_off;
  const float* p_pos; const float* p_head; const unsigned char* p_inv;
  const float* c_pos; const float* c_head; const unsigned char* c_inv; const unsigned char* c_ok; const int* c_src;
  const unsigned char* pair_ok;
  float radius; int K; int gap_rule; int index_diff;
  EdgeBuf e; int e_base;
};

struct MotionFeatArgs {
  const float* pos; const float* head; const int* state; const unsigned char* gap_mask;
  int rows, T;
  float* out;                       // [rows][T][4]
};

struct BuildEdgesArgs {
  SceneState st;
  int c;                            // current column
  int edgeless;                     // 1: write empty edge sets (column 0 chain)
  float r_map, r_agent;             // pl2a_radius, a2a_radius
  int rows;                         // S * A_cap
  EdgeBuf t, m, a;
  unsigned long long* prof;         // optional profiling counters (api.hip Prof::rows_dev): [8 + kind] += edges of the scene
  int map_lds;                      // float2 slots of dynamic LDS for the scene's map-token positions (0 .. 4096)
  unsigned long long* clear_keys;   // optional [rows]: k_heads' split arg-max keys, reset here when the k_integrate before ran in row groups
  int* clear_sync;                  // optional [S]: the per-scene counters of the k_layers_p launch that follows, zeroed here
};

struct RawFeatArgs {
  SceneState st;
  int col;
  const float* tok_tab;             // [3][token_size + 2][128]
  int token_size;
  const float* grid_tab;            // [grid_size + 1][128]
  int grid_size;
  const float* state_emb;           // [4][128]
  const float* cat_agent;           // [rows][128] type_emb[type] + shape_emb(shape)
  const float* cat_seed;            // [128]
  float* raw2;                      // [rows][4]  (|mv|, angle, -, -)
  float* cat;                       // [rows][128]
  float* fus_in;                    // [rows][512]
  const int* row_list; const int* row_mask; int n_list;   // optional: only these rows (row_mask[k] != 0), outputs compact at k
  int no_grid;                      // use_grid_token = False: fus_in columns 384..511 are not written (the fusion runs at K0 = 384)
};

struct IntegrateArgs {
  SceneState st;
  int c;                            // current column; writes column c + 1
  int t;                            // decode step
  int R;                            // num_recurrent_steps_val
  int force_valid;                  // disable_insertion: every state := valid
  int no_state;                     // use_state_token = False: 'exit' := valid after the ego override
  const int* next_token; const int* next_state;   // [rows] from the heads
  const int* teacher_token; const int* teacher_state;   // optional [S][T][A_cap]
  const int* teacher_grid;                               // optional [S][T][A_cap], < -1: none
  const float* teacher_pos; const float* teacher_head;   // optional [S][T][A_cap](x2): the stored pose of column c + 1
  const unsigned char* replay_row;                       // optional [S][A_cap]: teacher_* apply to the rows flagged 1 only (NULL: to every row)
  // the tail of a decode step folded into this launch (infgen_rollout_run with few rows; all optional):
  unsigned long long* heads_part;   // k_heads' split arg-max keys [rows]: decoded here (k_heads_finish) and reset for the next step
  int* next_token_w;                // where the decoded tokens go (the context's next_token array)
  int* edge_totals;                 // the three edge totals of the context, zeroed for the next column's k_build_edges
  int* zero_sync;                   // optional [S]: the per-scene counters of the next step's k_layers_p launch, zeroed here
  RawFeatArgs prep; int do_prep;    // the raw-feature gather (k_rawfeat_prep) of the new column, all rows of the scene
  int groups;                       // > 1: grid S x groups, A_cap / groups rows per workgroup (few scenes); the keys are then NOT reset here
  const float* vocab;               // [3][token_size][6][4][2]
  int token_size;
  const float* grid_xy; int grid_size;    // [G][2]
  float* pred_traj;                 // [S][A_cap][R][2]
  float* pred_head;                 // [S][A_cap][R]
  float* pred_state;                // [S][A_cap][R]
};


// edges into ONE query point per scene (insertion: the seed node at the ego pose, or a freshly
// inserted row during its heading stage): first-K agents / map tokens within a radius of the
// centre row's position, ascending index (torch_cluster.radius), filtered afterwards.
struct PointEdgesArgs {
  SceneState st;
  int c;
  const int* centre_row;            // [S] agent row whose column-c pose is the query point
  const int* active;                // [S] 0: emit nothing for this scene
  int exclude_centre;               // 1: the centre row is not a source (heading stage)
  int which;                        // bit 0: agents, bit 1: map tokens
  float r_agent; int k_agent;
  float r_map; int k_map;
  EdgeBuf ea, em;                   // one destination per scene: off[s], cnt[s]
};

struct InsertCatArgs {
  int S, A_cap;
  const int* inserted; const int* new_row; const int* type; const float* type_emb; const float* shp; const float* new_shape;
  float* cat_agent; float* shape_all; int* new_local;
};
struct OccupancyArgs { SceneState st; int c; int grid_size; float* occ; /* [S][grid_size] */ };
struct OccEmbedArgs { SceneState st; int c; int grid_size; float* occ; const float* pack; float* emb; /* [S][128] */
                      const int* active; /* optional: scenes with active[s] == 0 get the occupancy vector only */ };

struct InsertDecideArgs {
  SceneState st;
  int c, t, R, grid_size, force_enter, max_new;
  int sample_k; const float* uniform;   // cell sampling: top-k inverse CDF with uniform[S] (sample_k <= 1: arg-max)
  SamplingCtl ctl;                      // ... its temperature / top-p (scalars: temperature_row is not used per scene)
  const float* grid_xy;
  const float* lg_state;            // [S][2]
  const float* lg_type;             // [S][3]
  const float* shape;               // [S][3]
  const float* lg_pos;              // [S][grid_size]; k_insert_decide<false>: [S][2], seed_pos_rel_xy_predict_head (pre-tanh)
  float r_seed;                     // pl2seed_radius (k_insert_decide<false>)
  const float* occ;                 // [S][grid_size]
  int* n_agents;                    // [S] (mutable view of st.n_agents)
  int* type;                        // [S][A_cap]
  int* active;                      // [S] in/out
  int* n_new;                       // [S] in/out
  int* inserted;                    // [S] out
  int* new_row;                     // [S] out (global row index s*A_cap + a)
  float* new_shape;                 // [S][3] out
  int* new_cell;                    // [S] out
  float* pred_traj; float* pred_head; float* pred_state;
};

struct InsertFinalizeArgs {
  SceneState st;
  int c;
  float angle_interval;
  const int* inserted; const int* new_row;
  const float* lg_heading; int n_heading;     // [S][n_heading]
  const float* offset;                        // [S][2] (pre-tanh)
  float* hv_ovr;                              // [S][2]
};

struct SampleArgs {
  const float* logits; int rows; int n;      // [rows][n]
  int k;                                     // beam size (<= 16)
  const float* uniform;                      // [rows] caller-supplied U[0,1)
  int* token;                                // [rows] out
  float* sample_logprob;                     // optional [rows] out: log-probability of token[row] under the sampler's own distribution
  SamplingCtl ctl;                           // temperature / top-p
  int* nucleus;                              // optional [rows] out: the nucleus size m (k when top_p = 1; 1 on a greedy row)
};      // (k_sample_topk<true> takes Masked<SampleArgs>: banned columns are never picked; n a multiple of 32)

// the row's (1 / T, top_p) for topk_inverse_cdf, read once per row.  A greedy row (T == 0; anything below the smallest normal float
// counts: 1 / T of a denormal overflows, and 0 * inf would poison the row - the host entries refuse such values) is the
// nucleus of mass 0: m = 1, pick = 0, sum = exp(0) = 1, sample_logprob = 0 - the same code path, no branch of its own
__device__ __forceinline__ void sampling_row(const SamplingCtl& c, int row, float* it, float* top_p) {
  const float T = c.temperature_row ? c.temperature_row[row] : c.temperature;
  const bool drawn = T >= 1.17549435e-38f;      // FLT_MIN: 1 / T stays finite
  *it = drawn ? 1.0f / T : 1.0f;
  *top_p = drawn ? c.top_p : 0.f;
}

// the last block of top-k sampling, shared by k_sample_topk, k_heads_h<TERMS, LP, KS> and k_insert_decide so the three cannot drift
// apart.  topv[0..k-1]: the row's k best logits, descending; it = 1 / T; u01: the caller's uniform in [0, 1).
//   1. p[j] = expf((topv[j] - topv[0]) * it), cdf[j] the running sum in j order, S_k = cdf[k-1]
//   2. nucleus: the smallest m with cdf[m-1] >= top_p * S_k (top-k first, then top-p; m >= 1); top_p >= 1: m = k, no comparison
//   3. sum = cdf[m-1], u = u01 * sum, pick = the first j < m with u < cdf[j], else m - 1
// Returns pick; *sum_out = sum, *m_out = m.  The caller's sample_logprob is (topv[pick] - topv[0]) * it - logf(sum).
// With it = 1 and top_p = 1 this is the plain top-k draw bit for bit (x * 1.0f is exact, m = k, the additions keep their order).
// Statically indexed (KMAX rounds, guarded by k).
template <int KMAX>
__device__ __forceinline__ int topk_inverse_cdf(const float (&topv)[KMAX], int k, float u01, float it, float top_p, float* sum_out,
                                                int* m_out) {
  float p[KMAX], sum = 0.f;
#pragma unroll
  for (int j = 0; j < KMAX; ++j)
    if (j < k) { p[j] = expf((topv[j] - topv[0]) * it); sum += p[j]; }
  int m = k;
  if (top_p < 1.0f) {
    const float mass = top_p * sum;
    float c = 0.f;                       // the same additions in the same order: c after j rounds IS cdf[j-1]
    bool cut = false;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
      if (j < k && !cut) {
        c += p[j];
        if (c >= mass) { m = j + 1; cut = true; }
      }
    sum = c;
  }
  const float u = u01 * sum;
  float cdf = 0.f;
  int pick = m - 1;
  bool found = false;
#pragma unroll
  for (int j = 0; j < KMAX; ++j)
    if (j < m && !found) {
      cdf += p[j];
      if (u < cdf) { pick = j; found = true; }
    }
  *sum_out = sum;
  *m_out = m;
  return pick;
}

// topk_inverse_cdf under a token mask: with a allowed tokens the lists hold min(k, a) entries and TOPK_NONE columns behind them; the
// draw is over those min(k, a) only, so no uniform - 1 - 2^-24 and step 3's "else m - 1" included - lands on a slot without a token
template <int KMAX>
__device__ __forceinline__ int topk_inverse_cdf_masked(const float (&topv)[KMAX], const int (&topi)[KMAX], int k, float u01, float it,
                                                       float top_p, float* sum_out, int* m_out) {
  int live = 0;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) live += (j < k && topi[j] != TOPK_NONE) ? 1 : 0;
  return topk_inverse_cdf<KMAX>(topv, live > 1 ? live : 1, u01, it, top_p, sum_out, m_out);
}

// the row skeleton k_collision_mask and k_road_mask share (rider.cuh): one wave per row
constexpr int RIDER_WAVES = 4;          // rows a workgroup works on at a time (one wave each)
constexpr int RIDER_LIST = 128;         // reachable obstacles a wave keeps in LDS per pass over the row's tokens
constexpr int RIDER_WPL = 2;            // 32-token words a lane owns at most: token_size <= 64 * 32 * RIDER_WPL

// The argument block of a step rider or a closed-loop operator, in layers: the scene head every one of them reads, the mask head of
// the four mask riders on top of it, and the rider's RULE - its own parameters, the one definition its *Args inherits and its *Cfg
// (the configuration a registered mask carries; bits / out == NULL: none) embeds.  A rule's members lie in the order the
// infgen_token_mask_riders / infgen_token_mask_signal_get blocks export them
struct SceneHead {
  int S, A_cap, T;                      // the [S][T][A_cap] scene arrays (each block names its own column of them)
  const float* pos; const float* head; const int* state;      // [S][T][A_cap](x2)
  const int* n_agents; const int* type; const float* shape;   // [S], [S][A_cap], [S][A_cap][3] = (length, width, height)
};
struct MaskHead : SceneHead {           // (member order: the one under which the four mask kernels keep their register counts)
  const float* end_pose; int token_size;      // [3][token_size][4] = (dx, dy, cos, sin) + the three largest displacements
  const int* first_new;                 // optional [S]: rows >= first_new[s] were appended inside this step
  int* out_count; int c;                // optional [S * A_cap]; column c of the scene arrays is the current one
  unsigned* out_bits;                   // [S * A_cap][token_size / 32]
  TokenMaskCtl base;                    // the sets the rule refines (bits == NULL: every token)
};

// k_collision_mask (collision_kernels.hip): the per-step allowed-token sets of collision-aware decoding (include/infgen_hip.h, "collision
// masks"): set(i) = base(i) AND NOT collides(i) for every row of the layout, written as the row's own set of out_bits
constexpr int CM_STAGE = 9;             // floats the workgroup stages per obstacle row of the scene
struct CollisionRule { int predict; float margin; };
struct CollisionArgs : MaskHead, CollisionRule {
  int rows_per_wg;                      // rows of one scene a workgroup covers (a multiple of RIDER_WAVES)
};
struct CollisionCfg { unsigned* bits; const int* ident; const float* shape; const float* end_pose; CollisionRule rule; int* count; };
constexpr CollisionCfg COLLISION_NONE{nullptr, nullptr, nullptr, nullptr, {1, 0.f}, nullptr};
struct EndPoseArgs { const float* vocab; int token_size; float* end_pose; };     // vocab [3][token_size][6][4][2]
__global__ void k_collision_mask(CollisionArgs a);
__global__ void k_collision_end_poses(EndPoseArgs a);

// road_kernels.hip: the per-step allowed-token sets of road-aware decoding (include/infgen_hip.h, "road masks"):
// set(i) = base(i) AND NOT offroad(i), written as the row's own set of out_bits
constexpr int RM_REC = 8;               // floats of a record: anchor x, y, offset x, y | cos, sin, half length, radius
struct RoadRule {
  const float* paths;                                         // [3][token_size][4] = (cos, sin, half length, 0)
  const float* records; const int* n_records; int rec_cap;    // [S / copies][rec_cap][RM_REC], [S / copies]
  int copies, sweep; float margin; int types[3];              // types[ty] != 0: the rule applies to rows of agent type ty
};
struct RoadArgs : MaskHead, RoadRule {};
struct RoadCfg { unsigned* bits; const int* ident; const float* shape; const float* end_pose; RoadRule rule; int* count; };
constexpr RoadCfg ROAD_NONE{nullptr, nullptr, nullptr, nullptr, {nullptr, nullptr, nullptr, 0, 1, 1, 0.f, {0, 0, 0}}, nullptr};
struct RoadMapArgs {                    // k_road_records_map: one workgroup (one wave) per distinct scene
  const float* map_pos; const float* map_orient; const long long* map_type; const long long* map_tok; const int* n_map;   // [S0][M_cap](x2), [S0]
  int M_cap; const float* map_vocab; int n_token, detail;     // [n_token][11][2]
  float* records; int rec_cap; int* n_records;
};
struct RoadSegArgs { const float* segments; const int* n_segments; int E; float* records; int rec_cap; int* n_records; };
struct RoadPathArgs { const float* end_pose; int token_size; float* paths; };
__global__ void k_road_mask(RoadArgs a);
__global__ void k_road_records_map(RoadMapArgs a);
__global__ void k_road_records_seg(RoadSegArgs a);
__global__ void k_road_paths(RoadPathArgs a);

// route_kernels.hip: the per-step allowed-token sets of route-following decoding (include/infgen_hip.h, "route masks"):
// set(i) = base(i) AND onroute(i), written as the row's own set of out_bits
constexpr int RT_REC = 8;               // floats of a record: p0 x, y, direction x, y | L, cum, 0, 0
constexpr int RT_MAX_POINTS = 32;       // waypoints of a route at most: its segments fit the lanes of half a wave
struct RouteRule {
  const float* records; const float* total; int P;            // [S / copies][A_cap][P - 1][RT_REC], [S / copies][A_cap]
  int copies; float corridor, back, pace, finish; int types[3];      // types[ty] != 0: the rule applies to rows of agent type ty
};
struct RouteArgs : MaskHead, RouteRule {
  float* out_progress;                  // optional [S * A_cap][4] = s0, d0, total, flag
};
struct RouteCfg {
  unsigned* bits; const int* ident; const float* shape; const float* end_pose; RouteRule rule; int* count; float* progress;
};
constexpr RouteCfg ROUTE_NONE{nullptr, nullptr, nullptr, nullptr, {nullptr, nullptr, 2, 1, 0.f, 0.f, 0.f, 0.f, {0, 0, 0}}, nullptr, nullptr};
struct RouteRecArgs { const float* routes; const int* n_points; int rows, P; float* records; float* total; };   // rows = S * A_cap
__global__ void k_route_mask(RouteArgs a);
__global__ void k_route_records(RouteRecArgs a);

// signal_kernels.hip: the per-step allowed-token sets of signal-aware decoding (include/infgen_hip.h, "signal masks"):
// set(i) = base(i) AND NOT runs(i), written as the row's own set of out_bits
constexpr int SG_REC = 8;               // floats of a record: midpoint x, y, direction of lawful travel x, y | half length, 0, 0, 0
constexpr int SG_MAX_LINES = 64;        // stop lines of a map scene at most: one per lane of a wave
struct SignalRule {
  const float* records; const unsigned char* phase;           // [S / copies][K][SG_REC], [S / copies][n_phase][K]
  int n_phase, K;
  int copies; float setback, align; int types[3];             // types[ty] != 0: the rule applies to rows of agent type ty
};
struct SignalArgs : MaskHead, SignalRule {
  int t;                                // decode step t reads phase row t % n_phase
  float* out_info;                      // optional [S * A_cap][4] = gap, j, flag, 0
};
struct SignalCfg {
  unsigned* bits; const int* ident; const float* shape; const float* end_pose; SignalRule rule; int* count; float* info;
};
constexpr SignalCfg SIGNAL_NONE{nullptr, nullptr, nullptr, nullptr, {nullptr, nullptr, 1, 1, 1, 0.f, 0.f, {0, 0, 0}}, nullptr, nullptr};
struct SignalRecArgs { const float* lines; const int* n_lines; int S0, K; float* records; };
__global__ void k_signal_mask(SignalArgs a);
__global__ void k_signal_records(SignalRecArgs a);

// branch_kernels.hip: branching rollouts (include/infgen_hip.h, "branching").  k_branch_scenes gathers, for every scene s with a
// valid parent[s] != s, slot parent[s]'s rollout state into slot s - one launch over (chunk of a segment, scene).  A SEGMENT is one
// buffer of the context as `outer` blocks per scene: block o of scene s is the `bytes` bytes at base + o * outer_stride + s * bytes.
constexpr int BR_MAX_SEGS = 9 + 2 * INFGEN_MAX_LAYERS + 1 + 3 + 4;     // scene arrays, rings, X, pred_*, the three step-major logs, the score log
constexpr int BR_NT = 256;              // threads per workgroup
constexpr int BR_VEC = 4;               // 16-byte words a lane moves: all loads are issued before the first store
constexpr int BR_CHUNK = BR_NT * BR_VEC * 16;      // bytes of a block one workgroup moves
struct BranchSeg {
  char* base; long long bytes; long long outer_stride;
  int outer;                            // blocks per scene (ring slots, decode steps so far; 1 for the rest)
  int chunk0;                           // the segment's first chunk in the launch's x dimension (chunks per block = ceil(bytes / BR_CHUNK))
  int per_block;                        // chunks per block
  int wide;                             // 1: base, bytes and stride are multiples of 16 (16 bytes per lane), 0: byte by byte
};
struct BranchArgs {
  int S, n_seg;
  const int* parent; const int* map_scene;     // [S]; map_scene NULL: every scene is its own group
  int* n_bad;                                  // optional: entries treated as the identity
  BranchSeg seg[BR_MAX_SEGS];
};
struct ResampleArgs { const int* ancestor; int copies; int* parent; };      // [S0 * copies] each; one workgroup per group
constexpr int RS_NT = 256, RS_ITEMS = 4;       // copies <= RS_NT * RS_ITEMS
__global__ void k_branch_scenes(BranchArgs a);
__global__ void k_resample_parents(ResampleArgs a);

// snapshots (include/infgen_hip.h, "snapshots"): the same segments between the context and a caller's buffer of ENTRIES.  Entry e is the
// `stride` bytes at snap + e * stride; in it block o of segment k is the `bytes` bytes at entry_off[k] + o * align16(bytes) - segments in
// table order, every block on a 16-byte boundary.  k_snapshot_scenes<false>: (chunk, entry) - entry e := slot sel[e], head[e] written;
// k_snapshot_scenes<true>: (chunk, scene) - slot s := entry sel[s] where head[sel[s]] allows it.
struct SnapArgs {
  int S, n, t, n_seg;                          // scene slots, entries, the decode step of the boundary
  const int* sel;                              // save: slots [n]; restore: index [S]
  const int* map_scene;                        // [S] or NULL (a slot's group is the slot itself)
  int* head;                                   // [n][4] = slot, group, t, valid: written by the save, read by the restore
  char* snap; long long stride;
  int* n_bad;                                  // optional: entries skipped
  BranchSeg seg[BR_MAX_SEGS];
  long long entry_off[BR_MAX_SEGS];
};
template <bool RESTORE> __global__ void k_snapshot_scenes(SnapArgs a);

// score_kernels.hip: the step scores of one stored column (include/infgen_hip.h, "step scores"): 8 floats per scene slot, one flag byte
// per row
constexpr int SC_NT = 256;              // threads of the one workgroup per scene slot
struct ScoreRule {
  const float* records; const int* n_records; int rec_cap;    // [S / copies][rec_cap][RM_REC], [S / copies]; records NULL: no table
  int copies, sweep; float margin; int types[3]; float dt;
};
struct ScoreArgs : SceneHead, ScoreRule {
  int c1;                               // column c1 of the scene arrays is the scored one
  float* out; long long out_stride;     // slot s: the 8 floats at out + s * out_stride (32-byte aligned)
  unsigned char* out_row;               // optional [S][A_cap]: bit 0 live, bit 1 overlap, bit 2 off-road
};
struct ScoreCfg { float* out; int steps; unsigned char* row; const float* shape; ScoreRule rule; };      // steps: decode steps the log `out` holds
constexpr ScoreCfg SCORE_NONE{nullptr, 0, nullptr, nullptr, {nullptr, nullptr, 0, 1, 1, 0.f, {0, 0, 0}, 0.5f}};
__global__ void k_step_score(ScoreArgs a);

// observe_kernels.hip: the agent-frame observation of the rows named (include/infgen_hip.h, "observations"): own features, the K
// nearest live agents and the Km nearest map tokens of every row, one wave per row
constexpr int OB_WAVES = 4;             // rows a workgroup works on (one wave each)
constexpr int OB_LIST = 512;            // 64-bit keys a wave keeps in LDS; a fuller list is cut down to its K best first
constexpr int OBS_SELF = INFGEN_OBS_SELF, OBS_NBR = INFGEN_OBS_NBR, OBS_MAP = INFGEN_OBS_MAP, OBS_MAX_K = INFGEN_OBS_MAX_K;
static_assert(OBS_MAX_K <= 64 && OB_LIST >= 2 * 64, "one lane per selected entry; a cut-down list has room for 64 more");
struct ObserveArgs : SceneHead {
  int c;                                // column c of the scene arrays is the observed one
  float dt;
  const float* map_pos; const float* map_orient; const long long* map_type; const int* n_map;   // [S / copies][M_cap](x2), [S / copies]
  int M_cap, copies;
  const int* obs_row; int N, K, Km;     // optional [N] global rows s * A_cap + i (NULL: row n is n)
  float radius, map_radius;
  float* self_feat; float* nbr_feat; int* nbr_index; int* nbr_count;     // [N][8], [N][K][10], [N][K], [N]
  float* map_feat; int* map_index; int* map_count;                       // [N][Km][6], [N][Km], [N]
};
__global__ void k_observe_rows(ObserveArgs a);

// controller_kernels.hip: the target poses of rule-based controlled rows (include/infgen_hip.h, "IDM commands"): route projection,
// lead search and the car-following law, one wave per row
struct IdmArgs : SceneHead {
  int c;                                // column c of the scene arrays is the newest stored one, c >= 1
  const unsigned char* ctl_row;         // [S][A_cap]: != 0, the row is controlled
  const float* records; const float* total; int P, copies;    // [S / copies][A_cap][P - 1][RT_REC], [S / copies][A_cap]
  const float* v_des;                   // optional [S / copies][A_cap]: the row's own desired speed where > 0
  float dt, v0_type[3], headway, s_min, a_max, b_comf, b_max, lateral, keep;
  int types[3], stop_at_end;            // types[ty] != 0: rows of agent type ty may be ruled
  float* cmd_pose;                      // [S][A_cap][3], written for ruled rows only
  float* out_state; int* out_lead;      // optional [S * A_cap][8], [S * A_cap]
};
__global__ void k_idm_command(IdmArgs a);

struct TokenLogprobArgs {
  const float* logits; int rows; int n;      // [rows][n]
  const int* token;                          // [rows]
  float* out;                                // [rows]: logits[row][token] - logsumexp(row); 0 where token < 0
};

constexpr int MAP_GRAPH_C = 8;          // centre tokens per wave of k_map_graph (32 per workgroup: one LDS staging of the scene's tokens, one atomic)
struct MapGraphArgs {
  int S, M_cap; const int* n_map;
  const float* pos; const float* orient; float radius; int max_nbr;
  EdgeBuf e;
  int lds_tokens;          // tokens the launch's dynamic LDS holds (12 bytes each; 0: every trip reads global memory)
};

template <int W> __global__ void k_stream_read(const float* p, size_t n_floats, float* out);   // gemm_kernels.hip
__global__ void k_linear(LinearArgs a);
__global__ void k_linear_multi(LinearMultiArgs m);
__global__ void k_fourier(FourierArgs a);
template <int TERMS> __global__ void k_fourier_h(FourierArgs a);
template <int TERMS> __global__ void k_fourier_h_multi(FourierMultiArgs m);
template <int TERMS> __global__ void k_fourier_h12(FourierArgs a);      // fourier_h12.hip: three wave groups, 192-edge tiles
template <int TERMS> __global__ void k_fourier_h12_multi(FourierMultiArgs m);
constexpr int FH12_NT = 768, FH12_TILE = 192;
__global__ void k_match_tokens(MatchTokensArgs a);   // token_kernels.hip
template <int TERMS> __global__ void k_mlpemb_h(MlpEmbHArgs a);           // mlp_h.hip
__global__ void k_box_corners(NearestArgs a);        // metric_kernels.hip
__global__ void k_nearest_distance(NearestArgs a);
__global__ void k_kinematic(KinematicArgs a);
__global__ void k_ttc(TtcArgs a);
__global__ void k_placement(PlacementArgs a);
__global__ void k_window_loglik(WindowLoglikArgs a);
__global__ void k_bundle_field(BundleScoreArgs a);
__global__ void k_bundle_meta(BundleScoreArgs a);
__global__ void k_road_edge(RoadEdgeArgs a);
template <int TERMS, bool LP = false, int KS = 0, bool MK = false> __global__ void k_heads_h(ArgsFor<HeadsArgs, MK> a);   // LP: + token_logprob; KS > 0: + top-k sampling; MK: + token mask
template <int TERMS> __global__ void k_map_head_h(MapHeadArgs a);     // mlp_h.hip
template <int TERMS> __global__ void k_map_head_h_b16(MapHeadArgs a);
__global__ void k_map_topk(MapHeadArgs a);
__global__ void k_match_map_tokens(MatchMapArgs a);
__global__ void k_command_rows(CommandRowsArgs a);
__global__ void k_tokenize_prep(TokenizeArgs a);
__global__ void k_fetch_enterings(EnteringsArgs a);
__global__ void k_pt_grid_cells(EnteringsArgs a);
__global__ void k_tokenize_state(TokenizeArgs a);
__global__ void k_active_groups(ActiveGroupsArgs a);
template <int WAVES, int TERMS> __global__ void k_attn_h(AttnHArgs a);
// the *_b16 translation units: the same kernels with bf16-precision operands (gemm_terms = 2; TERMS = 1 only)
template <int WAVES, int TERMS> __global__ void k_attn_h_b16(AttnHArgs a);
template <int TERMS> __global__ void k_attn_hs_b16(AttnHArgs a);
template <int TERMS> __global__ void k_mlpemb_h_b16(MlpEmbHArgs a);
template <int TERMS, bool LP, int KS, bool MK> __global__ void k_heads_h_b16(ArgsFor<HeadsArgs, MK> a);          // (no default: mlp_h_b16.hip renames k_heads_h to this)
template <int TERMS> __global__ void k_fourier_h_b16(FourierArgs a);
template <int TERMS> __global__ void k_fourier_h_multi_b16(FourierMultiArgs m);
template <int TERMS> __global__ void k_attn_hs(AttnHArgs a);             // attn_hs.hip: the same for few rows (one 16-row group per workgroup)   // attn_h.hip     // fourier_h.hip: fp16 three-term split, register resident
__global__ void k_attn_pre(AttnPreArgs a);
__global__ void k_edge_attn(EdgeAttnArgs a);
template <int G> __global__ void k_edge_fused3(EdgeFusedArgs a);       // edge_fused3.hip: lane = (head, 16-column slice), rhat rows through LDS
template <int G, bool R24, int HALVES, int WAVES> __global__ void k_edge_fused(EdgeFusedArgs a);        // edge_fused.hip (R24: rhat rows in the packed format)
template <bool R24, int ROWS> __global__ void k_layers_p(LayersPArgs a);          // layers_p.hip
__global__ void k_edge_attn_wide(EdgeAttnArgs a);
__global__ void k_attn_post(AttnPostArgs a);
template <bool MK> __global__ void k_heads(ArgsFor<HeadsArgs, MK> a);
template <int BT> __global__ void k_build_edges(BuildEdgesArgs a);
template <int BT> __global__ void k_integrate(IntegrateArgs a);
__global__ void k_rawfeat_prep(RawFeatArgs a);
__global__ void k_scatter_rows(const float* src, const int* row_list, const int* row_mask, int n, float* dst);
__global__ void k_scatter_rows2(const float* src0, const float* src1, const int* row_list, const int* row_mask, int n, float* dst0,
                                float* dst1);
__global__ void k_note_riders(const int* new_row, const int* inserted, int n, int* prev_row, int* prev_mask, int* pend_row,
                              int* pend_mask);
struct EmbedSum4Args {
  const float* tab[4]; const long long* idx[4]; int n[4];
  int rows; float* out;
};
__global__ void k_embedding_sum4(EmbedSum4Args a);
__global__ void k_gather_rows(const float* src, const int* row_list, const int* row_mask, int n, int limit, float* dst);
__global__ void k_insert_cat(InsertCatArgs a);
__global__ void k_map_graph(MapGraphArgs a);
__global__ void k_point_edges(PointEdgesArgs a);
__global__ void k_occupancy(OccupancyArgs a);
__global__ void k_occupancy_embed(OccEmbedArgs a);
// insertion rules of the decision (include/infgen_hip.h, "insertion rules"): the masked instantiation k_insert_decide<true, true> takes
// the decision's argument block with these appended; the unmasked ones keep the block - and so their code - exactly as they were
struct InsertMaskCtl {
  const unsigned* allowed; int words;   // [S][words]: bit g set = cell g allowed (k_insert_cell_mask)
  int type_allowed[3];                  // vehicle, pedestrian, cyclist: 0 = never inserted
  const int* max_agents;                // optional [S]: no row is appended while live[s] >= max_agents[s]
  const int* live;                      // [S] (with max_agents): the rows in the scene at the step's column
  float* box_shape;                     // optional [S * A_cap][3]: the appended row's shape is written here too (the clearance rule's boxes)
};
struct InsertDecideMaskArgs : InsertDecideArgs { InsertMaskCtl m; };
// kGrid = false: use_grid_token = False (regressed world-frame position, no cell, no occupancy test); kMask: under insertion rules
template <bool kGrid, bool kMask = false>
__global__ void k_insert_decide(std::conditional_t<kMask, InsertDecideMaskArgs, InsertDecideArgs> a);

// k_insert_cell_mask (insert_mask_kernels.hip): the allowed cells of scenario insertion, one workgroup per scene
constexpr int IM_NT = 256;              // threads: wave w takes the 64-cell chunks w, w + 4, ..
constexpr int IM_TILE = 1024;           // entries (boxes, records, map tokens, zones) staged in LDS at a time; = MAX_SCENE_AGENTS
constexpr int IM_F = 6;                 // floats per staged entry
constexpr int IM_MAX_CELLS = 8192;      // a thread keeps one verdict bit per 256-cell round in a 32-bit register
enum { IM_KEEPOUT = 1, IM_CLEARANCE = 2, IM_EDGES = 4, IM_LANES = 8, IM_ZONES = 16 };
struct InsertCellMaskArgs {
  int S, A_cap, T, c, G, W;             // column c of the [S][T][A_cap] scene arrays; G cells, W words per scene
  const float* pos; const float* head; const int* state; const int* n_agents; const int* av_index;
  const float* shape;                   // [S * A_cap][3] = (length, width, height)
  const float* grid_xy;                 // [G][2], ego frame
  int rules;                            // IM_* bits
  int static_pass;                      // 0: static rules computed, not stored; 1: computed and stored; 2: read from static_bits
  float ko_back, ko_front, ko_half, clearance, edge_clearance, lane_dist;
  unsigned lane_types;                  // bit ty: map tokens of type ty count as lanes
  const float* records; const int* n_records; int rec_cap;
  const float* map_pos; const long long* map_type; const int* n_map; int M_cap;
  const float* zones; const int* n_zones; int Z;
  int copies;
  unsigned* static_bits; unsigned* allowed;     // [S][W]
  int* allowed_count; int* live;                // [S]
  int* count_log; long long count_stride;       // optional: count_log[s * count_stride] = allowed_count[s] as well
};
__global__ void k_insert_cell_mask(InsertCellMaskArgs a);
// kHeadToken = false: use_head_token = False (tanh * pi heading, unwrapped); kOffset = false: no xy offset (use_grid_token = False)
template <bool kHeadToken, bool kOffset> __global__ void k_insert_finalize(InsertFinalizeArgs a);
template <bool MK> __global__ void k_sample_topk(ArgsFor<SampleArgs, MK> a);
__global__ void k_token_logprob(TokenLogprobArgs a);
__global__ void k_layernorm(const float* X, int rows, const float* g, const float* b, float* Y);
__global__ void k_radius_edges(RadiusEdgesArgs a);            // forward_kernels.hip
__global__ void k_motion_features(MotionFeatArgs a);

// agent rows one scene can hold (INFGEN_Q_MAX_AGENTS); the ingest kernel's per-scene LDS tables are this long
constexpr int MAX_SCENE_AGENTS = 1024;
// ragged batch ingest / row pack (ingest_kernels.hip; the ingest's argument block is InfgenBatchIngest of include/infgen_hip.h)
constexpr int PACK_MAX_KEYS = 32;
struct PackRowsArgs {
  const char* src[PACK_MAX_KEYS]; char* dst[PACK_MAX_KEYS]; long long src_stride[PACK_MAX_KEYS];
  const int* counts[PACK_MAX_KEYS]; int count_stride[PACK_MAX_KEYS]; int row_bytes[PACK_MAX_KEYS];
  int n_keys, n_scenes, scene0, scene_step;
};
__global__ void k_ingest_batch(InfgenBatchIngest a);
__global__ void k_pack_rows(PackRowsArgs a);

// validation-step metrics and the open-loop loss (val_metrics.hip; reference infgen/utils/metrics.py).  Every kernel ADDS into a
// caller-owned accumulator of 8-byte slots: integer counters are int64 (integer atomics), floating sums are float64 reduced in a
// fixed order - rows inside a lane, lanes, then the workgroups' partials by k_vm_finish - without float atomics.
// Index arrays are int32 or int64 (the bool template arguments: true = int64), masks are bytes (torch.bool / uint8).
constexpr int VM_MAX_PARTIALS = 1024;     // workgroups of a float kernel; `scratch` holds VM_MAX_PARTIALS x 3 doubles
constexpr int GO_MAX_CELLS = 16384;       // cells the two LDS bitmaps of k_grid_overlap hold (the tokenizer's grid: 1961)
struct StateAccArgs {                // k_state_accuracy
  const void* state; const unsigned char* mask;            // [N][T] row strides ld / ldm (elements); mask may be null (part 1 only)
  int N, T; long long ld, ldm;
  int invalid_state, valid_state, enter_state, exit_state;
  unsigned long long* acc;                                  // [4]: valid, valid_count, invalid, invalid_count
};
struct GridOverlapArgs {             // k_grid_overlap
  const void* state; const void* grid;                      // [N][>= num_step], row strides lds / ldg
  long long lds, ldg;
  const long long* ptr;                                     // [n_group + 1] row ranges, or null: one group of all N rows
  int N, num_step, n_group, grid_size, enter_state, seed_size;
  unsigned long long* acc;                                  // [4][num_step]: overlap, insert, total, exceed_seed
};
struct TrajErrArgs {                 // k_traj_error
  const float* pred; const float* target; const unsigned char* valid;      // [N][T][2], [N][T][2], [N][T]
  int N, T;
  unsigned long long* ade_count; unsigned long long* fde_count;             // slot 1 of the two accumulators; either may be null
  double* partials;                                                         // [gridDim.x][2]: ade, fde
};
struct MaskedCeArgs {                // k_masked_ce
  const float* logits; long long ld;                        // [R][C], row stride ld
  const void* target; const unsigned char* mask; const float* weight;      // [R], [R], [C] or null
  int R, C, smooth;                                         // smooth: label smoothing != 0 (the all-class sum is needed)
  double* partials;                                         // [gridDim.x][3]
};
struct TokenClsArgs {                // k_token_cls
  const void* pred; long long ldp; int n_guess;             // [R][>= n_guess]
  const void* target; const unsigned char* mask;            // [R], [R]
  int R;
  unsigned long long* acc;                                  // [2]: sum, count
};
template <bool I64> __global__ void k_state_accuracy(StateAccArgs a);
template <bool S64, bool G64> __global__ void k_grid_overlap(GridOverlapArgs a);
__global__ void k_traj_error(TrajErrArgs a);
template <bool T64> __global__ void k_masked_ce(MaskedCeArgs a);
template <bool P64, bool T64> __global__ void k_token_cls(TokenClsArgs a);
__global__ void k_vm_sum(const float* val, long long n, double* partials, unsigned long long* count);   // AverageMeter: partial sums; *count += n
__global__ void k_vm_finish(const double* partials, int nb, int K, double* dst0, double* dst1, double* dst2);
constexpr int MTE_MAX_MODES = 64;    // modes per row of k_multi_traj_error (the top-k's taken set is one 64-bit word)
struct MultiTrajErrArgs {            // k_multi_traj_error (minMultiFDE.update / minMultiADE.update)
  const float* pred; const float* target; const float* prob; const unsigned char* valid;   // [N][M][T][2], [N][T][2], [N][M] or null, [N][T]
  int N, M, T, G;                                           // G: guesses used, 1 <= G <= M
  int keep_invalid_final_step, ade_by_ade;                  // row filter: any valid step / the last step; ADE criterion: 0 'FDE', 1 'ADE'
  unsigned long long* ade_count; unsigned long long* fde_count;             // slot 1 of the two accumulators; either may be null
  double* partials;                                                         // [gridDim.x][2]: ade, fde
};
__global__ void k_multi_traj_error(MultiTrajErrArgs a);

// modes from a scene's rollouts (mode_kernels.hip; reference batch_nms / new_batch_nms).  Row b = group g = b / rows_per_group, row
// r = b % rows_per_group of it; candidate j's step t starts at traj + g group_stride + r row_stride + j cand_stride + t step_stride
// (elements), F contiguous floats of which the first two are (x, y).
constexpr int SM_MAX_CAND = 64, SM_MAX_MODES = 16;
struct SelectModesArgs {             // k_select_modes
  const float* traj; long long group_stride, row_stride, cand_stride, step_stride;
  int rows_per_group; long long B; int N, T, F, t_goal, K;
  float dist_thresh;
  const float* score; int score_per_group;                  // [B][N] ([groups][N] with score_per_group), or null: density
  const unsigned char* cand_valid;                          // [B][N] or null
  const float* cand_state; long long state_group_stride, state_row_stride, state_cand_stride;   // optional: state at t_goal, unit step stride
  float state_invalid, state_enter;
  const int* row_limit; long long limit_stride;             // optional: row r of group g is valid while r < row_limit[g limit_stride]
  int* mode_idx; float* mode_score; float* mode_traj;       // [B][K], [B][K], [B][K][T][F] or null
};
__global__ void k_select_modes(SelectModesArgs a);

}  // namespace ig
