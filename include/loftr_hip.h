/* libloftr_hip -- C-ABI of the MI355X-native LoFTR matching path (gfx950 / CDNA4).
 *
 * Drop-in boundary.  The reference (zju3dv/LoFTR) is pure Python: it has no FFI / plugin
 * registry; the seam is nn.Module composition in src/loftr/loftr.py:20-27,56-75.  Each entry
 * point below replaces the ATen op sequence of one of those sub-modules and is what a ctypes
 * binding inside the reference's modules would call (INTEGRATION.md shows the stub).  The
 * Python mirror of the reference interface lives in loftr_amd/ and calls exactly these symbols.
 *
 * Conventions
 *   - every function is asynchronous on the caller-supplied hipStream_t (passed as void*);
 *   - all device buffers are caller-allocated (PyTorch owns memory); the library never
 *     allocates or frees device memory; `*_workspace_bytes` tells how much scratch to pass;
 *   - all floating point data is fp32 (GEMMs evaluate fp32 products as 3 fp16 MFMAs with fp32
 *     accumulation, csrc/gemm.h), ids are int64, masks are uint8 (0 = padded), as in the
 *     reference;
 *   - return value: 0 = ok, negative = loftr_status below (no exceptions);
 *   - no environment variable is read; the only process-global state are the debug switches, the timing mask and the
 *     range guard at the end of this header, all off / at their defaults unless set through their entry points.
 */
#ifndef LOFTR_HIP_H_
#define LOFTR_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  LOFTR_OK = 0,
  LOFTR_ERR_BAD_ARG = -1,       /* null pointer / non-positive or unsupported shape            */
  LOFTR_ERR_UNSUPPORTED = -2,   /* shape outside what the kernels are built for (C, H, D, W)   */
  LOFTR_ERR_WORKSPACE = -3,     /* workspace smaller than *_workspace_bytes()                  */
  LOFTR_ERR_LAUNCH = -4,        /* HIP reported a launch error                                 */
  LOFTR_ERR_NO_DEVICE = -5,     /* no gfx950 device visible                                    */
  LOFTR_ERR_COMM = -6,          /* RCCL unavailable or a collective / communicator call failed */
  LOFTR_ERR_RANGE = -7          /* range guard (loftr_hip_range_check_enable): |activation| >= 65504 or not finite */
} loftr_status;

/* 13: prepared transformer weights, RCCL entry points, scaled activations, pose estimation;
 * 14: training-side consumers (loftr_spvs_coarse / _fine, loftr_coarse_loss_sums, loftr_fine_loss_sums);
 * 16: backward of the matching heads and their losses (loftr_*_grad, loftr_dual_softmax_bwd, loftr_sinkhorn_bwd,
 *     loftr_fine_match_bwd);
 * 17: loftr_head_feat_grads (the feature-gradient GEMMs of both coarse heads);
 * 18: loftr_encoder_layer_bwd;
 * 19: loftr_fine_preprocess_bwd;
 * 20: loftr_conv_wgrad (backbone training: weight gradient of a convolution);
 * 21: training-mode glue of the backbone (loftr_bn_train_fwd / _bwd, loftr_act_fwd / _bwd, loftr_upsample2x_bilinear_fwd / _bwd);
 * 22: the persistent coarse transformer (loftr_coarse_plan_bytes / _build / _signature, loftr_transformer_fwd_planned) and the
 *     debug switches (loftr_hip_debug_set / _get) that replace the library's environment variables;
 * 23: loftr_conv_scratch_bytes / loftr_conv_bn_act_prepared_scratch (the 196-channel layers' remainder channels as a tap-decomposed product);
 * 24: loftr_transformer_fwd_padded (padding masks: 128-token tiles without a valid token are not computed);
 * 25: feature banks (loftr_pos_encode_flatten_gather, loftr_fine_preprocess_gather); later, without a bump (purely additive: a
 *     binding that needs them refuses a library without them when it loads): batched pose estimation on the GPU
 *     (loftr_estimate_pose_batched, loftr_estimate_pose_batched_workspace_bytes) and the fine head at matched windows only
 *     (loftr_window_head, loftr_fine_preprocess_window_head), homography / fundamental-matrix RANSAC (loftr_estimate_geometry,
 *     loftr_geometry_minimal, loftr_estimate_geometry_batched, loftr_estimate_geometry_batched_workspace_bytes), both convolutions
 *     of the fine head at matched windows (loftr_window_head_first, loftr_window_head_last, loftr_fine_preprocess_window_head2),
 *     absolute pose from matches and depth (loftr_estimate_absolute_pose, loftr_p3p, loftr_estimate_absolute_pose_batched,
 *     loftr_estimate_absolute_pose_batched_workspace_bytes, loftr_lift_keypoints), the keypoint atlas (loftr_atlas_*), triangulation
 *     of tracks (loftr_triangulate_tracks_host, loftr_triangulation_pairs, loftr_triangulate_tracks,
 *     loftr_triangulate_tracks_workspace_bytes), localisation against the triangulated model (loftr_model_cells_host,
 *     loftr_model_cells, loftr_model_lookup_host, loftr_model_lookup_workspace_bytes, loftr_model_lookup), bundle adjustment of the
 *     triangulated model (loftr_bundle_adjust_host, loftr_bundle_adjust_workspace_bytes, loftr_bundle_adjust; with per-image focal
 *     refinement loftr_bundle_adjust_focal_host, loftr_bundle_adjust_focal_workspace_bytes, loftr_bundle_adjust_focal; with one
 *     focal step per group of images loftr_bundle_adjust_shared_host, loftr_bundle_adjust_shared_workspace_bytes,
 *     loftr_bundle_adjust_shared; with position priors on the camera centres loftr_bundle_adjust_prior_host,
 *     loftr_bundle_adjust_prior_workspace_bytes, loftr_bundle_adjust_prior; with one radial coefficient per group of images
 *     loftr_bundle_adjust_radial_host, loftr_bundle_adjust_radial_workspace_bytes, loftr_bundle_adjust_radial, and the pixels without
 *     it loftr_undistort_points_host, loftr_undistort_points, loftr_distort_points_host), the correspondence table of the images without a pose (loftr_register_corr_host, loftr_register_corr_workspace_bytes,
 *     loftr_register_corr), track completion (loftr_complete_tracks_host, loftr_complete_tracks_workspace_bytes,
 *     loftr_complete_tracks), track merging (loftr_merge_tracks_host, loftr_merge_tracks_workspace_bytes, loftr_merge_tracks),
 *     3D similarity RANSAC and moving a model (loftr_estimate_similarity, loftr_similarity_minimal,
 *     loftr_estimate_similarity_batched_workspace_bytes, loftr_estimate_similarity_batched, loftr_transform_model_host,
 *     loftr_transform_model), track splitting (loftr_split_tracks_host, loftr_split_tracks_workspace_bytes, loftr_split_tracks), track
 *     refinement (loftr_refine_centres_host, loftr_refine_centres, loftr_fine_preprocess_gather_at), rotation averaging over the
 *     view graph (loftr_rotation_averaging_host, loftr_rotation_averaging_workspace_bytes, loftr_rotation_averaging) */
#define LOFTR_HIP_ABI_VERSION 25

int loftr_hip_abi_version(void);
const char* loftr_hip_status_string(int status);
/* 0 if the current HIP device is a gfx950 part, LOFTR_ERR_NO_DEVICE otherwise. */
int loftr_hip_device_check(void);

/* A 4-D feature map [N,C,H,W] addressed through element strides (sn,sc,sh,sw), so that both NCHW
 * and channels-last (what the MIOpen backbone produces fastest) storage work without a copy. */
typedef struct {
  const float* data;
  long sn, sc, sh, sw;    /* element strides */
  int H, W;               /* spatial size    */
} loftr_fmap;

/* ---- position encoding + flatten ---------------------------------------------------------
 * Replaces: PositionEncodingSine.forward (src/loftr/utils/position_encoding.py:37-42) followed
 * by rearrange 'n c h w -> n (h w) c' (src/loftr/loftr.py:58-59).
 *   feat: [N,C,H,W] map (any strides), pe [C,pe_h,pe_w] (the module's constant table, H<=pe_h,
 *   W<=pe_w), out [N,H*W,C] contiguous. */
int loftr_pos_encode_flatten(const loftr_fmap* feat, const float* pe, int pe_h, int pe_w,
                             float* out, int N, int C, void* stream);

/* ---- LoFTREncoderLayer / LocalFeatureTransformer ------------------------------------------
 * Weights of one LoFTREncoderLayer (src/loftr/loftr_module/transformer.py:7-33); every matrix
 * is the nn.Linear weight as stored in the state_dict: [out_features, in_features] row-major. */
typedef struct {
  const float* q_proj;   /* [C, C]   */
  const float* k_proj;   /* [C, C]   */
  const float* v_proj;   /* [C, C]   */
  const float* merge;    /* [C, C]   */
  const float* mlp0;     /* [2C, 2C] */
  const float* mlp2;     /* [C, 2C]  */
  const float* norm1_w;  /* [C] */
  const float* norm1_b;  /* [C] */
  const float* norm2_w;  /* [C] */
  const float* norm2_b;  /* [C] */
} loftr_layer_weights;

/* Scratch needed by loftr_encoder_layer_fwd / loftr_transformer_fwd for `nb` sequences of
 * length L attending to sequences of length S (transformer: pass nb = 2*N). */
size_t loftr_encoder_workspace_bytes(int nb, int L, int S, int C);

/* Replaces: LoFTREncoderLayer.forward (transformer.py:35-58) incl. LinearAttention.forward
 * (src/loftr/loftr_module/linear_attention.py:20-47).
 *   x [nb,L,C], source [nb,S,C], x_mask [nb,L] / source_mask [nb,S] uint8 or NULL,
 *   out [nb,L,C] (may alias x).  C in {128, 256}, H = 8. */
int loftr_encoder_layer_fwd(const float* x, const float* source, const uint8_t* x_mask,
                            const uint8_t* source_mask, const loftr_layer_weights* w, float* out,
                            int nb, int L, int S, int C, int H, void* ws, size_t ws_bytes,
                            void* stream);

/* Backward of loftr_encoder_layer_fwd (what torch.autograd derives from transformer.py:35-58 + linear_attention.py:20-47):
 * from grad_out = dL/d out [nb,L,C]:  grad_x [nb,L,C], grad_source [nb,S,C] (WRITTEN, not accumulated: a self layer's caller adds
 * the two) and the gradients of the ten weight tensors (written into the caller's buffers, shapes as loftr_layer_weights).
 * The layer is recomputed from (x, source) in the workspace; C in {128, 256}, head dimension 16 or 32. */
typedef struct {
  float* q_proj; float* k_proj; float* v_proj; float* merge; float* mlp0; float* mlp2;
  float* norm1_w; float* norm1_b; float* norm2_w; float* norm2_b;
} loftr_layer_grads;
size_t loftr_encoder_layer_bwd_workspace_bytes(int nb, int L, int S, int C, int H);
int loftr_encoder_layer_bwd(const float* x, const float* source, const uint8_t* x_mask, const uint8_t* source_mask,
                            const loftr_layer_weights* w, const float* grad_out, float* grad_x, float* grad_source,
                            const loftr_layer_grads* gw, int nb, int L, int S, int C, int H, void* ws, size_t ws_bytes,
                            void* stream);

/* Replaces: LocalFeatureTransformer.forward (transformer.py:80-101), in place on feat0/feat1.
 *   feat0 [N,L,C], feat1 [N,S,C]; layer_is_cross[i] = 0 for 'self', 1 for 'cross';
 *   cross layers keep the reference's sequential dependency (feat1 attends to the UPDATED
 *   feat0, :96-97).  When L == S and feat1 == feat0 + N*L*C the two self-attention calls of a
 *   layer run as one batch of 2N sequences. */
int loftr_transformer_fwd(float* feat0, float* feat1, const uint8_t* mask0, const uint8_t* mask1,
                          const loftr_layer_weights* layers, const int* layer_is_cross,
                          int n_layers, int N, int L, int S, int C, int H, const void* prepared,
                          size_t prepared_bytes, void* ws, size_t ws_bytes, void* stream);
/* loftr_transformer_fwd for a caller that does not read the features of PADDING tokens (mask byte 0; MegaDepth batches padded to a common
 * size, dataset.py:107-125).  The reference computes x + LayerNorm2(mlp([x, b1])) for them in every layer, and nothing in LoFTR.forward reads
 * it: their scores are filled (coarse_matching.py:115-118), as attention sources they are multiplied by zero (linear_attention.py:37-40) and
 * the fine stage only gathers at matched -- valid -- tokens.  With skip_padded_tiles != 0 and masks given, a 128-token tile (tokens
 * 128 t .. 128 t + 127 of a sequence) whose mask bytes are all zero keeps its INPUT values in feat0 / feat1; every other token comes out
 * bit-identical to loftr_transformer_fwd (a fully masked tile's K^T V / Ksum partial is exactly +0 and is written as such in either call).
 * skip_padded_tiles == 0 or no masks: the same as loftr_transformer_fwd. */
int loftr_transformer_fwd_padded(float* feat0, float* feat1, const uint8_t* mask0, const uint8_t* mask1,
                                 const loftr_layer_weights* layers, const int* layer_is_cross,
                                 int n_layers, int N, int L, int S, int C, int H, const void* prepared,
                                 size_t prepared_bytes, void* ws, size_t ws_bytes, int skip_padded_tiles, void* stream);
/* The same forward as ONE persistent launch (csrc/encoder_fused.hip: coarse_persistent_kernel).  The reference's schedule
 * (transformer.py:91-99) synchronises whole calls; its data dependency -- feat1 attends to the UPDATED feat0 -- is per pair, and
 * below that per 128-token tile.  A PLAN is the dependency graph of one forward's work items for a shape (n_layers of the pattern
 * [self, cross] * P, N pairs, L and S tokens), ordered by a list schedule on the host; 256 resident workgroups pull it in order and
 * wait on counters in the workspace.  Build it once per shape into a caller-owned DEVICE buffer of loftr_coarse_plan_bytes() bytes
 * (0 = shape not supported; loftr_coarse_plan_build is a set-up call: it synchronises the stream), then pass it here.
 *   order 0 = dependency-driven (critical path first), 1 = the reference's call order (same arithmetic item by item: results are
 *   bit-identical, tests/test_hip_parity.py); the same value must be given to _build and to _fwd_planned.
 *   diag: NULL, or a device buffer of diag_bytes >= 16: word 0 = error (0 ok; 2 = the plan was built for another shape / order and
 *   nothing was computed; odd = a workgroup gave up waiting for a dependency after ~1 s, value = 1 + 2 * item), words 1-3 reserved;
 *   with diag_bytes >= 16 + 32 * items (items = loftr_coarse_plan_bytes / 32 - 1) additionally per work item four 8-byte words
 *   {popped, dependencies met, done} in 10 ns ticks and the workgroup id (profiling).  The caller zeroes word 0.
 * C = 256, H = 8, n_layers <= 8 even; anything else: LOFTR_ERR_UNSUPPORTED (use loftr_transformer_fwd). */
size_t loftr_coarse_plan_bytes(const int* layer_is_cross, int n_layers, int N, int L, int S);
int loftr_coarse_plan_build(const int* layer_is_cross, int n_layers, int N, int L, int S, int order, void* plan,
                            size_t plan_bytes, void* stream);
unsigned loftr_coarse_plan_signature(int n_layers, int N, int L, int S, int order);
int loftr_transformer_fwd_planned(float* feat0, float* feat1, const uint8_t* mask0, const uint8_t* mask1,
                                  const loftr_layer_weights* layers, const int* layer_is_cross,
                                  int n_layers, int N, int L, int S, int C, int H, const void* prepared,
                                  size_t prepared_bytes, void* ws, size_t ws_bytes, const void* plan,
                                  size_t plan_bytes, int plan_order, void* diag, size_t diag_bytes, void* stream);

/* Inference with constant weights: every layer matrix is re-encoded once (row-scaled split-fp16 operand format,
 * csrc/gemm.h) into a caller-owned buffer of loftr_transformer_prepared_bytes(n_layers, C) bytes; hand it to
 * loftr_transformer_fwd as `prepared` (NULL there = convert on every call into the workspace).  The LayerNorm vectors
 * are always read from `layers`.  The buffer must be rebuilt when a weight changes. */
size_t loftr_transformer_prepared_bytes(int n_layers, int C);
int loftr_transformer_prepare(const loftr_layer_weights* layers, int n_layers, int C, void* prepared,
                              size_t prepared_bytes, void* stream);

/* ---- CoarseMatching ------------------------------------------------------------------------
 * Geometry + selection parameters shared by the two match types. */
typedef struct {
  int N, h0c, w0c, h1c, w1c;     /* L = h0c*w0c, S = h1c*w1c                                    */
  int C;                         /* descriptor width (256)                                      */
  float thr;                     /* config['thr']            (strict >)                         */
  int border_rm;                 /* config['border_rm']                                          */
  float scale;                   /* hw0_i[0] / hw0_c[0]      (coarse_matching.py:242)           */
  const uint8_t* mask0;          /* [N,L] or NULL (MegaDepth padding masks)                     */
  const uint8_t* mask1;          /* [N,S] or NULL                                               */
  const float* scale0;           /* [N,2] or NULL                                               */
  const float* scale1;           /* [N,2] or NULL                                               */
} loftr_coarse_params;

/* Match outputs; capacity must be N*L rows (at most one match per row of conf_matrix).
 * counts[0] = M (total), counts[1+b] = matches of pair b.  Rows are in ascending (b, i). */
typedef struct {
  int64_t* b_ids;     /* [N*L] */
  int64_t* i_ids;     /* [N*L] */
  int64_t* j_ids;     /* [N*L] */
  float* mconf;       /* [N*L] */
  float* mkpts0_c;    /* [N*L,2] */
  float* mkpts1_c;    /* [N*L,2] */
  int32_t* counts;    /* [1+N]   */
} loftr_match_out;

size_t loftr_coarse_match_workspace_bytes(int N, int L, int S, int C);

/* Replaces: CoarseMatching.forward, match_type='dual_softmax' + get_coarse_match, eval branch
 * (src/loftr/utils/coarse_matching.py:105-119,150-196,238-261).
 *   feat_c0 [N,L,C], feat_c1 [N,S,C]; conf_out [N,L,S] or NULL (data['conf_matrix'] elided). */
int loftr_coarse_match_dual_softmax(const float* feat_c0, const float* feat_c1,
                                    const loftr_coarse_params* p, float temperature,
                                    float* conf_out, const loftr_match_out* out, void* ws,
                                    size_t ws_bytes, void* stream);

/* Replaces: CoarseMatching.forward, match_type='sinkhorn' (coarse_matching.py:121-143, calling
 * SuperGlue's log_optimal_transport) + get_coarse_match.
 *   conf_out [N,L,S] REQUIRED (used as the score store); assign_out [N,L+1,S+1] or NULL
 *   (data['conf_matrix_with_bin'] when config['sparse_spvs']). */
int loftr_coarse_match_sinkhorn(const float* feat_c0, const float* feat_c1,
                                const loftr_coarse_params* p, float bin_score, int iters,
                                int prefilter, float* conf_out, float* assign_out,
                                const loftr_match_out* out, void* ws, size_t ws_bytes,
                                void* stream);

/* ---- FinePreprocess ------------------------------------------------------------------------
 * Replaces: FinePreprocess.forward (src/loftr/loftr_module/fine_preprocess.py:29-59): 5x5
 * windows (stride = hf/hc, zero padded) of the fine maps at the matched cells, fused with the
 * down-projected coarse features.  No unfold volume is materialised.
 *   feat_f0/1: fine maps (loftr_fmap, any strides; channels-last reads are fully coalesced);
 *   feat_c0 [N,L,Cc], feat_c1 [N,S,Cc] (transformer outputs);
 *   out0/out1 [M,W*W,Cf].  down_w [Cf,Cc], down_b [Cf], merge_w [Cf,2Cf], merge_b [Cf];
 *   (fine_concat_coarse_feat = False -- down_w NULL -- is not supported: no shipped config uses it.) */

size_t loftr_fine_preprocess_workspace_bytes(int M, int W, int Cf);

int loftr_fine_preprocess(const loftr_fmap* feat_f0, const loftr_fmap* feat_f1,
                          const float* feat_c0, const float* feat_c1, int L, int S, int Cc,
                          const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M,
                          int w0c, int w1c, int stride, int W, int Cf,
                          const float* down_w, const float* down_b, const float* merge_w,
                          const float* merge_b, float* out0, float* out1, void* ws,
                          size_t ws_bytes, void* stream);

/* Backward of loftr_fine_preprocess (fine_preprocess.py:29-59 under autograd) from grad_out0 / grad_out1 [M, W*W, Cf].
 *   grad_f0 / grad_f1 (maps laid out like feat_f0 / feat_f1), grad_c0 [N,L,Cc], grad_c1 [N,S,Cc]: ADDED TO (zero-fill them first:
 *   windows overlap and a cell may carry several matches; float atomics).  The four parameter gradients are written. */
size_t loftr_fine_preprocess_bwd_workspace_bytes(int M, int W, int Cf, int Cc);
int loftr_fine_preprocess_bwd(const loftr_fmap* feat_f0, const loftr_fmap* feat_f1, const float* feat_c0, const float* feat_c1,
                              int L, int S, int Cc, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M,
                              int w0c, int w1c, int stride, int W, int Cf, const float* down_w, const float* down_b,
                              const float* merge_w, const float* grad_out0, const float* grad_out1, const loftr_fmap* grad_f0,
                              const loftr_fmap* grad_f1, float* grad_c0, float* grad_c1, float* grad_down_w, float* grad_down_b,
                              float* grad_merge_w, float* grad_merge_b, void* ws, size_t ws_bytes, void* stream);

/* ---- feature banks (ABI 25) ----------------------------------------------------------------
 * A bank is one loftr_fmap whose batch index is a SLOT: the backbone maps of many images, each extracted once, matched in any
 * pairing (loftr_amd/pairs.py: FeatureBank, LoFTR.match_pairs).  Slot ids are int32 device arrays; slot offsets are computed
 * in 64 bits, so a bank may hold more than 2^31 elements.  Same per-element arithmetic as the entry points they mirror: a
 * pair matched through a bank gives the bits of the same pair matched from stacked maps.  A slot id outside [0, n_slots)
 * reads nothing and yields NaN outputs (callers validate ids on the host; the binding refuses them before any launch).
 * n == 0 / M == 0 is a no-op success; null pointers otherwise return LOFTR_ERR_BAD_ARG.
 *
 * loftr_pos_encode_flatten_gather: out[r] = flatten(bank[slot_ids[r]] + pe) for r < n, out [n, H*W, C] contiguous.
 *   bank: [n_slots, C, H, W] (any strides; channels-last reads are coalesced), slot_ids [n]. */
int loftr_pos_encode_flatten_gather(const loftr_fmap* bank, int n_slots, const int32_t* slot_ids, int n,
                                    const float* pe, int pe_h, int pe_w, float* out, int C, void* stream);

/* loftr_fine_preprocess with the fine maps read from banks: the window of match m comes from bank_f0[slot0[b_ids[m]]] /
 * bank_f1[slot1[b_ids[m]]] instead of feat_f0[b_ids[m]] / feat_f1[b_ids[m]].  slot0 / slot1 [N] map the batch-local pair b to
 * the bank slot of each side (the two banks may differ, hence one n_slots per side); feat_c0 / feat_c1 stay per pair.  Every
 * other argument, and the workspace (loftr_fine_preprocess_workspace_bytes), as for loftr_fine_preprocess. */
int loftr_fine_preprocess_gather(const loftr_fmap* bank_f0, int n_slots0, const int32_t* slot0,
                                 const loftr_fmap* bank_f1, int n_slots1, const int32_t* slot1,
                                 const float* feat_c0, const float* feat_c1, int L, int S, int Cc,
                                 const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M,
                                 int w0c, int w1c, int stride, int W, int Cf,
                                 const float* down_w, const float* down_b, const float* merge_w,
                                 const float* merge_b, float* out0, float* out1, void* ws,
                                 size_t ws_bytes, void* stream);

/* ---- the fine head at matched windows only (ABI 25, additive) ------------------------------------------
 * The fine map has one consumer in the inference forward: the W x W windows of FinePreprocess.  These entry points evaluate the
 * LAST convolution of the FPN fine head (3x3, stride 1, pad 1, no BatchNorm, no activation) only at the window pixels and write
 * the windows directly -- no fine map.  Bit for bit the windows loftr_fine_preprocess gathers from the dense convolution's output
 * (same MFMA, same k order, same epilogue expression).
 *   h_sp0 / h_sp1: output of the head's FIRST convolution (+ BN + LeakyReLU) for the image0 / image1 batch, SP [N, H, Wm, ceil32(Cin)]
 *                  (both batches of one size; they may be the two halves of one tensor);
 *   prepared:      the second convolution's filter from loftr_conv_prepare (Cin, Cout, 3, 3, no BatchNorm).
 * Supported: W = 5, ceil32(Cout) = 128; anything else returns LOFTR_ERR_UNSUPPORTED (callers take the dense head).
 *
 * loftr_window_head: the windows alone, win0_sp / win1_sp SP [M, W*W, 128] (the GEMM operand format of the library).
 * loftr_fine_preprocess_window_head: loftr_fine_preprocess with the windows computed this way; every other argument, and the
 *   workspace (loftr_fine_preprocess_workspace_bytes), as there.  Cf = Cout. */
int loftr_window_head(const uint32_t* h_sp0, const uint32_t* h_sp1, int N, int H, int Wm, int Cin,
                      const void* prepared, size_t prepared_bytes, int Cout, const int64_t* b_ids,
                      const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int W,
                      uint32_t* win0_sp, uint32_t* win1_sp, void* stream);
int loftr_fine_preprocess_window_head(const uint32_t* h_sp0, const uint32_t* h_sp1, int N, int H, int Wm, int Cin,
                                      const void* prepared, size_t prepared_bytes,
                                      const float* feat_c0, const float* feat_c1, int L, int S, int Cc,
                                      const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M,
                                      int w0c, int w1c, int stride, int W, int Cf,
                                      const float* down_w, const float* down_b, const float* merge_w,
                                      const float* merge_b, float* out0, float* out1, void* ws, size_t ws_bytes,
                                      void* stream);

/* ---- both convolutions of the fine head at matched windows only (ABI 25, additive) ----------------------
 * The output of the head's FIRST convolution (3x3, stride 1, pad 1, BatchNorm, LeakyReLU 0.01) is read by loftr_window_head at
 * the 7 x 7 neighbourhood of each window only.  loftr_window_head_first evaluates it there, from the FPN top-down map:
 *   t_sp0 / t_sp1: input of the head for the image0 / image1 batch, SP [N, H, Wm, ceil32(Cin)];
 *   prepared:      the first convolution's folded filter from loftr_conv_prepare (Cin, Cout, 3, 3, with its BatchNorm);
 *   nb_sp:         SP [2 M, 49, ceil32(Cout)]: window w = side * M + m, row py * 7 + px = the dense layer's SP row of pixel
 *                  (y0 - 1 + py, x0 - 1 + px), (y0, x0) the window's top-left pixel; ZERO words for pixels outside the map (the
 *                  second convolution's zero padding) and in the pad channels.  Bit for bit the dense layer's words.
 * loftr_window_head_last: loftr_window_head reading those rows instead of the dense map (prepared: the second filter).
 * loftr_fine_preprocess_window_head2: loftr_fine_preprocess_window_head with both convolutions computed this way (prepared0 /
 *   prepared1: first / second filter, Cmid the channels between them); nb_sp is caller-owned scratch of 2 M * 49 * ceil32(Cmid) dwords.
 * Supported: W = 5, channels 196 -> 196 -> 128, 2 M * 49 * 224 < 2^31; anything else returns LOFTR_ERR_UNSUPPORTED. */
int loftr_window_head_first(const uint32_t* t_sp0, const uint32_t* t_sp1, int N, int H, int Wm, int Cin,
                            const void* prepared, size_t prepared_bytes, int Cout, const int64_t* b_ids,
                            const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int W,
                            uint32_t* nb_sp, void* stream);
int loftr_window_head_last(const uint32_t* nb_sp, int H, int Wm, int Cin, const void* prepared, size_t prepared_bytes,
                           int Cout, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M, int w0c,
                           int w1c, int stride, int W, uint32_t* win0_sp, uint32_t* win1_sp, void* stream);
int loftr_fine_preprocess_window_head2(const uint32_t* t_sp0, const uint32_t* t_sp1, int N, int H, int Wm, int Cin,
                                       const void* prepared0, size_t prepared0_bytes, int Cmid,
                                       const void* prepared1, size_t prepared1_bytes,
                                       const float* feat_c0, const float* feat_c1, int L, int S, int Cc,
                                       const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M,
                                       int w0c, int w1c, int stride, int W, int Cf,
                                       const float* down_w, const float* down_b, const float* merge_w,
                                       const float* merge_b, float* out0, float* out1, void* ws, size_t ws_bytes,
                                       uint32_t* nb_sp, void* stream);

/* ---- FineMatching ---------------------------------------------------------------------------
 * Replaces: FineMatching.forward + get_fine_match (src/loftr/utils/fine_matching.py:15-74).
 *   feat_f0/1 [M,WW,C]; mkpts1_c [M,2]; b_ids [M]; scale = hw0_i[0]/hw0_f[0];
 *   scale1 [N,2] or NULL (applied iff the batch has 'scale0', fine_matching.py:68);
 *   expec_f [M,3] (x, y, std), mkpts1_f [M,2].  (mkpts0_f is mkpts0_c, :66.) */
int loftr_fine_match(const float* feat_f0, const float* feat_f1, int M, int WW, int C,
                     const float* mkpts1_c, const int64_t* b_ids, float scale,
                     const float* scale1, float* expec_f, float* mkpts1_f, void* stream);

/* ---- ResNet-FPN building blocks (the caller side of the path) -----------------
 * Activations are NHWC tensors in the library's SP GEMM-operand format: uint32 [B, H, W, Cp] with
 * Cp = C rounded up to a multiple of 32; per 32-channel group 16 dwords of fp16 "hi" halves then 16 dwords
 * of fp16 "lo" halves (x ~= hi + lo, csrc/gemm.h); pad channels are zero.  loftr_sp_from_f32 /
 * loftr_sp_to_f32 convert from / to plain fp32 NHWC.
 *
 * loftr_conv_bn_act replaces nn.Conv2d (bias=False) [+ eval-mode nn.BatchNorm2d] [+ residual add]
 * [+ ReLU / LeakyReLU] of src/loftr/backbone/resnet_fpn.py:5-40,100-118 as ONE implicit-GEMM kernel:
 *   x_sp [B,H,W,ceil32(Cin)], weight [Cout,Cin,KH,KW] fp32 as in the state_dict, addressed through its four
 *   element strides (contiguous or channels-last storage), bn_* [Cout] or all NULL,
 *   act: 0 none, 1 ReLU, 2 LeakyReLU(0.01); residual_sp [B,Ho,Wo,ceil32(Cout)] or NULL (added before act);
 *   outputs y_sp (SP) and / or y_f32 (fp32 [B,Ho,Wo,Cout]); Ho = (H + 2 pad - KH) / stride + 1.
 * loftr_upsample2x_add replaces F.interpolate(scale_factor=2, bilinear, align_corners=True) + add (:111-116). */
size_t loftr_conv_workspace_bytes(int Cin, int Cout, int KH, int KW);
int loftr_conv_bn_act(const uint32_t* x_sp, int B, int H, int W, int Cin, const float* weight,
                      const long* weight_strides, int Cout, int KH, int KW, int stride, int pad, const float* bn_weight, const float* bn_bias,
                      const float* bn_mean, const float* bn_var, float bn_eps, int act,
                      const uint32_t* residual_sp, uint32_t* y_sp, float* y_f32, void* ws, size_t ws_bytes,
                      const float* x_inv_scale, void* stream);
/* Inference with constant weights: fold BN + encode the filter once, then run any number of convolutions on it.
 * loftr_conv_prepare fills `prepared` (loftr_conv_workspace_bytes(Cin, Cout, KH, KW) bytes, caller-owned, must
 * stay untouched while in use); loftr_conv_bn_act_prepared is loftr_conv_bn_act (low_sp == NULL) or
 * loftr_conv1x1_upsample_add (low_sp != NULL: 1x1 / stride 1 / no act / SP output only) without the per-call
 * weight preparation (two launches and a memset per convolution).  loftr_conv_bn_act == prepare into ws + this. */
int loftr_conv_prepare(const float* weight, const long* weight_strides, int Cin, int Cout, int KH, int KW,
                       const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var,
                       float bn_eps, void* prepared, size_t prepared_bytes, void* stream);
/* OR-ed into `act` of loftr_conv_bn_act / loftr_conv_bn_act_prepared: this launch shares the GPU with work on another
 * stream (e.g. the FPN fine branch next to the coarse matching stage).  The 3x3 kernel then launches one workgroup per
 * tile instead of one persistent workgroup per CU: a persistent workgroup holds its CU (151 KB of LDS) for the whole
 * kernel, so the other stream could only start between kernels; with per-tile workgroups it interleaves every ~50 us
 * (measured: +1 % end to end with the two-stream overlap, -1.2 % on the kernel when it runs alone). */
#define LOFTR_CONV_SHARED_GPU 0x100
int loftr_conv_bn_act_prepared(const uint32_t* x_sp, int B, int H, int W, int Cin, const void* prepared,
                               size_t prepared_bytes, int Cout, int KH, int KW, int stride, int pad, int act,
                               const uint32_t* residual_sp, const uint32_t* low_sp, uint32_t* y_sp, float* y_f32,
                               const float* x_inv_scale, void* stream);
/* The same with a SCRATCH buffer (round 6, ABI 23).  3x3 / stride-1 layers whose output width is 193 .. 199 channels (LoFTR's 196) pad to 224
 * columns: the 7th 32-column tile spends a whole tile's matrix work on <= 7 real channels.  With loftr_conv_scratch_bytes(..) bytes of scratch
 * (0 = this shape has no such form) those channels are computed as a TAP-DECOMPOSED product instead -- conv = sum over the nine taps of shifted
 * 1x1 convolutions, so all (tap, channel) pairs are the columns of ONE K = Cin product on the unshifted pixels, evaluated at the centre-tap
 * steps of the main kernel into the scratch (fp32 [pixels][9 R]) and summed, shifted, by a second small kernel (csrc/conv3x3_duo.h).  Same
 * products, another summation order for those channels (fp32 noise).  scratch == NULL or too small, y_f32 requested, debug switch
 * "conv_rem" = 0: exactly loftr_conv_bn_act_prepared. */
size_t loftr_conv_scratch_bytes(int B, int H, int W, int Cout, int KH, int KW, int stride);
int loftr_conv_bn_act_prepared_scratch(const uint32_t* x_sp, int B, int H, int W, int Cin, const void* prepared,
                                       size_t prepared_bytes, int Cout, int KH, int KW, int stride, int pad, int act,
                                       const uint32_t* residual_sp, const uint32_t* low_sp, uint32_t* y_sp, float* y_f32,
                                       const float* x_inv_scale, void* scratch, size_t scratch_bytes, void* stream);
/* Stem: nn.Conv2d(1, C0, 7, stride 2, padding 3, bias=False) + eval BatchNorm2d + ReLU (resnet_fpn.py:52-54,101),
 * direct convolution; x [B,1,H,W] fp32 through its element strides (sb, sc, sh, sw), y_sp [B,Ho,Wo,ceil32(C0)]. */
int loftr_stem_conv_bn_relu(const float* x, const long* x_strides, int B, int H, int W, const float* weight,
                            const long* weight_strides, int C0, const float* bn_weight, const float* bn_bias,
                            const float* bn_mean, const float* bn_var, float bn_eps, uint32_t* y_sp, void* stream);
int loftr_upsample2x_add(const uint32_t* low_sp, const uint32_t* lateral_sp, uint32_t* out_sp, int B, int Hl,
                         int Wl, int C, void* stream);
/* One FPN top-down step (resnet_fpn.py:110-112 / :115-117) in one launch:
 *   y = conv1x1(x, weight) + F.interpolate(low, scale_factor=2, mode='bilinear', align_corners=True)
 * x_sp [B,H,W,ceil32(Cin)], weight [Cout,Cin,1,1] (bias-free lateral `layerK_outconv`), low_sp
 * [B,H/2,W/2,ceil32(Cout)], y_sp [B,H,W,ceil32(Cout)]; H and W even.  The lateral map never reaches HBM
 * and is added in fp32 (the two-call form rounds it to SP first).  Workspace: loftr_conv_workspace_bytes(Cin,Cout,1,1). */
int loftr_conv1x1_upsample_add(const uint32_t* x_sp, int B, int H, int W, int Cin, const float* weight,
                               const long* weight_strides, int Cout, const uint32_t* low_sp, uint32_t* y_sp,
                               void* ws, size_t ws_bytes, void* stream);
int loftr_sp_from_f32(const float* src, uint32_t* dst_sp, long rows, int C, void* stream);
/* Operand scaling (csrc/gemm.h).  The fp16 (hi, lo) pair keeps 22 bits of a value only above 2^-3; GEMM operands are
 * therefore stored times a power of two that lifts their maximum to [2^13, 2^14).  Filters: per output channel, inside
 * loftr_conv_prepare.  Activations produced by the library are BatchNorm / LayerNorm bounded and stored as they are; an
 * fp32 activation tensor of arbitrary magnitude enters through loftr_sp_from_f32_scaled, which writes the INVERSE of the
 * power of two it applied to the whole tensor to *inv_scale_out (device float) -- pass that pointer as x_inv_scale to
 * loftr_conv_bn_act / loftr_conv_bn_act_prepared (NULL = the tensor is unscaled). */
int loftr_sp_from_f32_scaled(const float* src, uint32_t* dst_sp, long rows, int C, float* inv_scale_out, void* stream);
int loftr_sp_to_f32(const uint32_t* src_sp, float* dst, long rows, int C, void* stream);

/* ---- evaluation caller (the reference's test_step, src/lightning/lightning_loftr.py:205-229) ----------
 * Replaces compute_symmetrical_epipolar_errors (src/utils/metrics.py:50-68 with :31-47): squared symmetric
 * epipolar distance of every match under the ground-truth relative pose of its pair, fp32.
 *   mkpts0_f / mkpts1_f [M,2] f32 pixels, m_bids [M] i64 pair index, T_0to1 [N,4,4], K0 / K1 [N,3,3] f32
 *   (row-major), epi_errs [M] f32 in match order (= the reference's per-pair concatenation, because the matcher
 *   emits matches grouped by ascending pair).  A match whose pair index is outside [0,N) gets NaN. */
int loftr_epipolar_errors(const float* mkpts0_f, const float* mkpts1_f, const long* m_bids, const float* T_0to1,
                          const float* K0, const float* K1, long M, int N, float* epi_errs, void* stream);

/* ---- training-side consumers of the path's outputs, FORWARD VALUES ONLY --------------------
 * loftr_spvs_coarse replaces spvs_coarse (src/loftr/utils/supervision.py:22-109, with warp_kpts of
 * src/loftr/utils/geometry.py:5-54): both coarse grids are warped into the other image through the depth maps and the
 * relative pose, rounded to the nearest coarse cell, and the mutual-nearest pairs become the ground-truth matches.
 *   depth0 [N,dh0,dw0], depth1 [N,dh1,dw1] f32; T_0to1, T_1to0 [N,4,4]; K0, K1 [N,3,3]; scale0/1 [N,2] or NULL (both);
 *   mask0 [N,L], mask1 [N,S] uint8 coarse masks or NULL (both); H*, W* = image sizes, scale = RESOLUTION[0] (8).
 *   Outputs: w_pt0_i [N,L,2], pt1_i [N,S,2] (data['spv_w_pt0_i'], ['spv_pt1_i']); spv_b/i/j [capacity N*L] in ascending
 *   (b, i), *count = their number (device int32; 0 -> the caller substitutes the reference's single (0,0,0), :94-99);
 *   conf_gt [N,L,S] or NULL (data['conf_matrix_gt']; the losses below work from the id lists and do not need it).
 * loftr_spvs_fine replaces spvs_fine (:124-142): expec_f_gt = (w_pt0_i[b,i] - pt1_i[b,j]) / scale / radius, scale
 *   multiplied by scale1[b] when given (the reference applies it iff 'scale0' is in the batch).
 * loftr_coarse_loss_sums / loftr_fine_loss_sums produce the reduction sums of LoFTRLoss (src/losses/loftr_loss.py:22-157)
 *   in fp64, one pass each (see csrc/train.hip for the layout of `sums`); the means, weights and corner cases are
 *   finished by the caller (loftr_amd/training.py).  Their gradients: loftr_coarse_loss_grad / loftr_fine_loss_grad below. */
typedef struct {
  int N, H0, W0, H1, W1, scale;
  int dh0, dw0, dh1, dw1;
  const float* depth0; const float* depth1;
  const float* T_0to1; const float* T_1to0;
  const float* K0; const float* K1;
  const float* scale0; const float* scale1;
  const uint8_t* mask0; const uint8_t* mask1;
} loftr_spvs_params;
size_t loftr_spvs_coarse_workspace_bytes(int N, int L, int S);
int loftr_spvs_coarse(const loftr_spvs_params* p, float* w_pt0_i, float* pt1_i, int64_t* spv_b, int64_t* spv_i, int64_t* spv_j,
                      int32_t* count, float* conf_gt, void* ws, size_t ws_bytes, void* stream);
int loftr_spvs_fine(const float* w_pt0_i, const float* pt1_i, int L, int S, const int64_t* b_ids, const int64_t* i_ids,
                    const int64_t* j_ids, long M, float scale, float radius, const float* scale1, float* expec_f_gt, void* stream);
size_t loftr_loss_workspace_bytes(int N, int L, int S);
int loftr_coarse_loss_sums(const float* conf, int N, int L, int S, int kind, const int64_t* gt_b, const int64_t* gt_i,
                           const int64_t* gt_j, long M, const uint8_t* mask0, const uint8_t* mask1, float alpha, float gamma,
                           double* sums, void* ws, size_t ws_bytes, void* stream);
int loftr_fine_loss_sums(const float* expec_f, int ld, const float* expec_f_gt, long M, int with_std, float correct_thr,
                         double* sums, void* ws, size_t ws_bytes, void* stream);

/* ---- backward of the matching heads and of the losses that read them -----------------------------------------------
 * What torch.autograd derives for the reference between `loss` (src/lightning/lightning_loftr.py:112-133,
 * src/losses/loftr_loss.py:165-192) and the INPUTS OF THE TWO HEADS: feat_c0 / feat_c1 entering CoarseMatching
 * (src/loftr/utils/coarse_matching.py:105-119, dual-softmax) and feat_f0 / feat_f1 entering FineMatching
 * (src/loftr/utils/fine_matching.py:43-57).  One kernel per node; each recomputes the forward quantities it needs from the
 * node's inputs.  Upstream of the heads the chain continues with loftr_encoder_layer_bwd, loftr_fine_preprocess_bwd and
 * loftr_conv_wgrad (+ the forward convolutions on the transposed filter for the input gradient) declared further down.
 *
 * loftr_coarse_loss_grad: grad_conf = d(pos_scale * sum_pos + neg_scale * sum_neg) / d conf for the sums of
 *   loftr_coarse_loss_sums with the same kind, ids and masks ([N,L,S]; kind 1: [N,L+1,S+1] = conf_matrix_with_bin, workspace
 *   loftr_loss_workspace_bytes); the gradient of torch.clamp(conf, 1e-6, 1 - 1e-6) (:45,:54) is included.  The caller folds
 *   means, loss weights, corner cases (:31-42) and the upstream gradient into pos_scale = up * c_pos_w / M and neg_scale =
 *   up * c_neg_w / (N L S - M) (kind 1: / sums[3], the number of supervised dustbin entries).
 * loftr_fine_loss_grad: grad_expec [M,ld] = upstream * d loss_f / d expec_f (:108-157); `sums` is the DEVICE array the forward
 *   (loftr_fine_loss_sums) filled; the std column gets 0 (weight.detach(), :131); training = the module's .training (:113-117).
 * loftr_dual_softmax_bwd: dsim [N,L,S] = dL/d sim_matrix from grad_conf = dL/d conf_matrix (:110-119; 0 on the mask-filled
 *   entries).  sim = <feat_c0, feat_c1> / (C * temperature), so dL/dfeat_c0 = dsim . feat_c1 / (C T) and dL/dfeat_c1 =
 *   dsim^T . feat_c0 / (C T): loftr_head_feat_grads below (split-fp16 MFMA, csrc/head_grads.hip).
 *   Workspace: loftr_coarse_match_workspace_bytes(N, L, S, C).
 * loftr_fine_match_bwd: grad_f0 / grad_f1 [M,WW,C] from grad_expec [M,3] = dL/d expec_f (x, y, std) (:43-57; grad_f0 is
 *   non-zero at the centre row only, :43).
 * loftr_sinkhorn_bwd: the Sinkhorn head (coarse_matching.py:121-143 + SuperGlue log_optimal_transport) in reverse mode through
 *   the `iters` unrolled iterations: dZ [N,L+1,S+1] = dL/d couplings (scores padded with bin_score) from grad_assign =
 *   dL/d conf_matrix_with_bin, *dbin = dL/d bin_score (device float); z_scratch [N,L,S] receives the re-created scores.
 *   sim = <feat_c0, feat_c1> / C: the caller slices dZ[:, :L, :S] (zero on mask-filled entries) and finishes with two GEMMs. */
int loftr_coarse_loss_grad(const float* conf, int N, int L, int S, int kind, const int64_t* gt_b, const int64_t* gt_i,
                           const int64_t* gt_j, long M, const uint8_t* mask0, const uint8_t* mask1, float alpha, float gamma,
                           double pos_scale, double neg_scale, float* grad_conf, void* ws, size_t ws_bytes, void* stream);
int loftr_fine_loss_grad(const float* expec_f, int ld, const float* expec_f_gt, long M, int with_std, float correct_thr,
                         int training, const double* sums, float upstream, float* grad_expec, void* stream);
int loftr_dual_softmax_bwd(const float* feat_c0, const float* feat_c1, const loftr_coarse_params* p, float temperature,
                           const float* grad_conf, float* dsim, void* ws, size_t ws_bytes, void* stream);
int loftr_fine_match_bwd(const float* feat_f0, const float* feat_f1, int M, int WW, int C, const float* grad_expec,
                         float* grad_f0, float* grad_f1, void* stream);
/* The einsum behind both coarse heads in reverse (coarse_matching.py:110-114 / :122-123: sim = <feat_c0, feat_c1> * alpha):
 *   g0 [N,L,C] = alpha * dsim . feat_c1,   g1 [N,S,C] = alpha * dsim^T . feat_c0       (either output may be null)
 * dsim: N matrices of L x S floats with row pitch dsim_ld and batch stride dsim_bs (the Sinkhorn head hands in the interior of its
 * [L+1, S+1] gradient); fp32 in and out, split-fp16 MFMA products with fp32 accumulation (csrc/head_grads.hip).  C % 32 == 0, C <= 256. */
int loftr_head_feat_grads(const float* dsim, long dsim_ld, long dsim_bs, const float* feat_c0, const float* feat_c1,
                          int N, int L, int S, int C, float alpha, float* g0, float* g1, void* stream);
/* Weight gradient of a bias-free convolution (what autograd computes for every nn.Conv2d of resnet_fpn.py in a training step):
 *   dw_taps[ky * KW + kx][co][ci] = sum_{b,y,x} dy[b,y,x,co] * x[b, y stride + ky - pad, x stride + kx - pad, ci]   (zero outside the map)
 * dy [B,Ho,Wo,Cout], x [B,H,W,Cin] fp32 channels-last; the caller permutes dw_taps [KH*KW, Cout, Cin] to [Cout,Cin,KH,KW].  All taps in
 * one launch, each a split-K product over the output pixels on the split-fp16 MFMA path with fp32 accumulation and an ordered sum of the partials
 * (deterministic).  Cin % 4 == 0, Cin <= 256 (the one-channel stem: hand in the 7 x 7 patches as a 52-channel 1 x 1 problem).
 * The input gradient is loftr_conv_bn_act on the flipped, transposed filter (stride 2: on the zero-interleaved dy). */
size_t loftr_conv_wgrad_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int KH, int KW);
int loftr_conv_wgrad(const float* dy, const float* x, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                     float* dw_taps, void* ws, size_t ws_bytes, void* stream);
size_t loftr_sinkhorn_bwd_workspace_bytes(int N, int L, int S, int C, int iters);
int loftr_sinkhorn_bwd(const float* feat_c0, const float* feat_c1, const loftr_coarse_params* p, float bin_score, int iters,
                       const float* grad_assign, float* z_scratch, float* dZ, float* dbin, void* ws, size_t ws_bytes, void* stream);

/* Replaces estimate_pose (src/utils/metrics.py:72-98: cv2.findEssentialMat(RANSAC) + cv2.recoverPose on intrinsics-
 * normalised key points), the pose step of compute_pose_errors (:101-136).  HOST function (cv2 is a CPU library too):
 * all pointers are host memory, the call is synchronous.  kpts0 / kpts1 [M,2] pixels, K0 / K1 [3,3] row-major,
 * thresh_px = RANSAC_PIXEL_THR (0.5), conf = RANSAC_CONF (0.99999), seed for the sampler.
 * Outputs: R [3,3], t [3] (unit norm), inliers [M] (RANSAC inliers that are in front of both cameras), *n_inliers =
 * their number, or -1 when the reference would return None (M < 5, no model, no point passes the cheirality test).
 * PARITY UNPINNED against OpenCV (absent from this image): published algorithms restated (five-point solver of Nister
 * 2004, Sampson-distance RANSAC with OpenCV's documented parameters), own sampling sequence -- csrc/pose.hip.
 * loftr_five_point exposes the minimal / least-squares solver: q0 / q1 [n,2] normalised points (double), up to 10
 * essential matrices (row-major, unit Frobenius norm) in E_out [10,9]. */
int loftr_estimate_pose(const float* kpts0, const float* kpts1, long M, const float* K0, const float* K1, float thresh_px,
                        float conf, unsigned seed, float* R_out, float* t_out, uint8_t* inliers_out, long* n_inliers);
int loftr_five_point(const double* q0, const double* q1, int n, double* E_out, int* n_solutions);

/* loftr_estimate_pose for every pair of a batch, on the GPU (csrc/pose_gpu.hip).  CONTRACT: for every pair p the result is
 * the one loftr_estimate_pose returns for that pair's matches with the same seed -- same n_inliers, same inlier mask, R and t
 * equal after the float32 rounding.  Parity against OpenCV stays UNPINNED, as for the host estimator.
 *   mkpts0_f / mkpts1_f [M,2] f32 pixels, m_bids [M] i64: device memory, grouped by ascending pair id as the matcher emits
 *   them (pair p = the matches with m_bids == p, in match order); K0 / K1 [P,3,3] f32 row-major, device memory;
 *   thresh_px, conf: as loftr_estimate_pose; seed: one seed shared by every pair (compute_pose_errors uses 0).
 * Outputs (device memory): R_out [P,9], t_out [P,3] f32; inliers_out [M] u8 in match order (RANSAC inliers in front of both
 * cameras); n_inliers [P] i64 = their number, or -1 where loftr_estimate_pose returns -1 (fewer than 5 matches, no model, no
 * point passes the cheirality test) -- there R, t and the pair's mask are 0.
 * Stream-ordered on `stream`; the keypoints never leave the device.  The call copies the per-hypothesis inlier counts to the
 * host once, replays the RANSAC loop there (the host estimator's own pow / log) and waits for the stream before it returns:
 * two host round trips per batch, whatever P.  Workspace: loftr_estimate_pose_batched_workspace_bytes(M, P), about 830 kB
 * per pair plus 33 bytes per match.
 * Status: LOFTR_ERR_BAD_ARG for a null pointer, M < 0 or P < 0, P == 0 with M > 0, and for m_bids outside [0, P) or not
 * grouped by ascending pair (found on the device, reported at the call's own synchronisation; the outputs are then not
 * written); LOFTR_ERR_WORKSPACE for a short workspace; LOFTR_ERR_UNSUPPORTED for M >= 2^31 or P >= 2^31 / 1000.
 * M == 0 is valid (every pair gets -1); P == 0 and M == 0 is a no-op success. */
size_t loftr_estimate_pose_batched_workspace_bytes(long M, int P);
int loftr_estimate_pose_batched(const float* mkpts0_f, const float* mkpts1_f, const long* m_bids, long M, const float* K0,
                                const float* K1, int P, float thresh_px, float conf, unsigned seed, float* R_out, float* t_out,
                                uint8_t* inliers_out, long* n_inliers, void* ws, size_t ws_bytes, void* stream);

/* Geometric verification without intrinsics: a homography (model 0: x1 ~ H x0) or a fundamental matrix (model 1: x1^T F x0 = 0)
 * by RANSAC over minimal solvers and a least-squares refit (csrc/geometry.hip; what cv2.findHomography(RANSAC) /
 * cv2.findFundamentalMat(FM_RANSAC) are used for on planar and on uncalibrated pairs).  HOST function: all pointers are host
 * memory, the call is synchronous.  kpts0 / kpts1 [M,2] pixels; thresh_px and every residual are in pixels.
 *   Sampling: loftr_estimate_pose's own -- xorshift64* from `seed`, distinct indices, at most 1000 iterations, a hypothesis
 *   replaces the best only with strictly more inliers, the adaptive stop log(1 - conf) / log(1 - w^s) with sample size s = 4 (H)
 *   or 7 (F).  The sample stream does not depend on the scores.
 *   Solvers (fp64, Hartley normalisation of the s sample points per image): H = null vector of the 8 x 9 DLT matrix; a sample is
 *   rejected when any three of its four points are collinear in either image -- |signed area| of the triple (twice the
 *   triangle's area, measured in the normalised frame of the four points: centroid 0, mean distance sqrt 2) below 1e-3 -- or when a
 *   triple's orientation differs between the images.  F = the up to three real roots of det(a F1 + (1 - a) F2) = 0 over the two
 *   null vectors of the 7 x 9 matrix.
 *   Residuals: H squared forward transfer error |x1 - pi(H x0)|^2 (a match whose H x0 has a non-positive third coordinate, with
 *   the sign that makes it positive at the sample, is an outlier); F squared Sampson distance.  Inlier: residual <= thresh_px^2.
 *   Refit: normalised least squares over the inliers of the best hypothesis (rank 2 enforced for F; skipped for F with fewer than
 *   8 inliers), adopted when it has at least as many inliers, and repeated on the adopted model's inliers while it strictly gains
 *   inliers (at most 4 fits: the adaptive stop can end on a hypothesis that holds only part of the inliers).  Its sums run in a fixed order (256 strided partials, partial k over
 *   the matches i = k mod 256 in ascending i, then a pairwise tree), which the GPU estimator reproduces.
 * Outputs: mat_out [9] row-major with unit Frobenius norm and a fixed sign (H: positive third coordinate of H x0 at the inliers;
 * F: the entry of largest magnitude positive), inliers_out [M] and *n_inliers of the returned model; *n_inliers = -1 (outputs
 * untouched) when M < s, no sample gave a model, or the best model has fewer than s inliers.
 * PARITY UNPINNED against OpenCV (absent from this image): published algorithms restated, own sampling sequence and degeneracy
 * tests.
 * loftr_geometry_minimal exposes the minimal solvers: p0 / p1 [s,2] pixels (double) -> up to 3 matrices in mats_out [3,9]. */
int loftr_estimate_geometry(const float* kpts0, const float* kpts1, long M, int model, float thresh_px, float conf, unsigned seed,
                            float* mat_out, uint8_t* inliers_out, long* n_inliers);
int loftr_geometry_minimal(const double* p0, const double* p1, int model, double* mats_out, int* n_solutions);

/* loftr_estimate_geometry for every pair of a batch, on the GPU (csrc/geometry_gpu.hip).  CONTRACT: for every pair p the result
 * is the one loftr_estimate_geometry returns for that pair's matches with the same seed and model -- same n_inliers, same inlier
 * mask, the matrix equal after the float32 rounding.  Parity against OpenCV stays UNPINNED, as for the host estimator.
 *   mkpts0_f / mkpts1_f [M,2] f32 pixels, m_bids [M] i64: device memory, grouped by ascending pair id as the matcher emits
 *   them (pair p = the matches with m_bids == p, in match order); model, thresh_px, conf: as loftr_estimate_geometry; seed: one
 *   seed shared by every pair.
 * Outputs (device memory): mat_out [P,9] f32; inliers_out [M] u8 in match order; n_inliers [P] i64, or -1 where
 * loftr_estimate_geometry returns -1 -- there the matrix and the pair's mask are 0.
 * Stream-ordered on `stream`; the keypoints never leave the device.  The call copies the per-hypothesis inlier counts to the
 * host once, replays the RANSAC loop there (the host estimator's own pow / log), copies one decision per pair back and waits for
 * the stream before it returns: two host round trips per batch, whatever P.  Workspace:
 * loftr_estimate_geometry_batched_workspace_bytes(M, P, model), about 96 kB (H) / 270 kB (F) per pair plus 33 bytes per match.
 * Status: LOFTR_ERR_BAD_ARG for a null pointer, M < 0 or P < 0, model outside {0, 1}, P == 0 with M > 0, and for m_bids outside
 * [0, P) or not grouped by ascending pair (found on the device, reported at the call's own synchronisation; the outputs are then
 * not written); LOFTR_ERR_WORKSPACE for a short workspace; LOFTR_ERR_UNSUPPORTED for M >= 2^31 or P >= 2^31 / 1000.
 * M == 0 is valid (every pair gets -1); P == 0 and M == 0 is a no-op success. */
size_t loftr_estimate_geometry_batched_workspace_bytes(long M, int P, int model);
int loftr_estimate_geometry_batched(const float* mkpts0_f, const float* mkpts1_f, const long* m_bids, long M, int P, int model,
                                    float thresh_px, float conf, unsigned seed, float* mat_out, uint8_t* inliers_out,
                                    long* n_inliers, void* ws, size_t ws_bytes, void* stream);

/* Absolute pose (camera resection, PnP) from 2D-3D matches: x_cam = R X + t by P3P inside RANSAC and a Gauss-Newton refit on the
 * pixel reprojection error (csrc/absolute_pose.hip; what cv2.solvePnPRansac is used for when one image of the pair has a depth map:
 * InLoc / Aachen localisation, RGB-D re-localisation).  The result is metric -- in the units of the 3D points -- and does not
 * degenerate on planar scenes or small baselines as the five-point path does.  HOST function: all pointers are host memory, the call
 * is synchronous.  pts3d [M,3] points (any rigid frame), kpts [M,2] pixels of the camera to resect, K [3,3] its intrinsics: upper
 * triangular (fx, skew, cx, fy, cy are read; K[2] is taken as (0, 0, 1)).  thresh_px and every residual are in pixels.
 *   Sampling: loftr_estimate_pose's own -- xorshift64* from `seed`, 3 distinct indices, at most 1000 iterations, a hypothesis replaces
 *   the best only with strictly more inliers (the solutions of one sample in solver order), the adaptive stop
 *   log(1 - conf) / log(1 - w^3).  The sample stream does not depend on the scores.
 *   Solver (fp64): unit bearings f = K^-1 (u, v, 1) by the closed-form inverse; Grunert's P3P as in Haralick et al. (IJCV 1994): the
 *   quartic in the depth ratio v = s3 / s1, its real positive roots by the Aberth-Ehrlich + Newton finder, the three distances
 *   polished by 4 Newton steps on the cosine-law equations (a solution is kept when each holds to 1e-10 x the longest squared side),
 *   R and t from the orthonormal frames of the two point triples.  Up to 4 poses.  Degenerate samples give none:
 *   |(P2 - P1) x (P3 - P1)|^2 <= (1e-6)^2 x (longest squared side)^2 (collinear world points), or |f_i x f_j|^2 <= (1e-7)^2 for two
 *   of the bearings (coincident bearings).  Both rules are relative (scale-free).
 *   Residual: p = K (R X + t); inlier iff p_z > 0 and |(p_x / p_z, p_y / p_z) - kpt|^2 <= thresh_px^2.
 *   Refit: 5 Gauss-Newton steps on the reprojection error over the inliers of the best hypothesis (left rotation increment applied
 *   through the normalised quaternion (1, w / 2), additive translation; a non-positive pivot of the 6 x 6 elimination fails the fit
 *   and keeps the current model; skipped below 4 inliers), adopted when it has at least as many inliers, and repeated on the adopted
 *   model's inliers while it strictly gains inliers (at most 4 fits).  Its 27 sums run in a fixed order (256 strided partials,
 *   partial k over the matches i = k mod 256 in ascending i, then a pairwise tree), which the GPU estimator reproduces.
 * Outputs: R_out [9] row-major, t_out [3], inliers_out [M] and *n_inliers of the returned model; *n_inliers = -1 with R, t and the mask
 * zero when M < 3, no sample gave a model, or the best model has fewer than 3 inliers.
 * PARITY UNPINNED against OpenCV's solvePnPRansac (absent from this image): published algorithms restated, own sampling sequence and
 * degeneracy tests.
 * loftr_p3p exposes the minimal solver: X [3,3] world points, bearings [3,3] (normalised by the call) -> n_solutions <= 4 poses in
 * R_out [4,9] / t_out [4,3] (double). */
int loftr_estimate_absolute_pose(const float* pts3d, const float* kpts, long M, const float* K, float thresh_px, float conf, unsigned seed,
                                 float* R_out, float* t_out, uint8_t* inliers_out, long* n_inliers);
int loftr_p3p(const double* X, const double* bearings, double* R_out, double* t_out, int* n_solutions);

/* loftr_estimate_absolute_pose for every pair of a batch, on the GPU (csrc/absolute_pose_gpu.hip).  CONTRACT: for every pair p the
 * result is the one loftr_estimate_absolute_pose returns for that pair's matches and K[p] with the same seed -- same n_inliers, same
 * inlier mask, R and t equal after the float32 rounding.  Parity against OpenCV stays UNPINNED, as for the host estimator.
 *   pts3d [M,3] f32, kpts [M,2] f32 pixels, m_bids [M] i64, K [P,3,3] f32: device memory; the matches grouped by ascending pair id as
 *   the matcher emits them (pair p = the matches with m_bids == p, in match order); thresh_px, conf: as the host estimator; seed: one
 *   seed shared by every pair.
 * Outputs (device memory): R_out [P,9], t_out [P,3] f32; inliers_out [M] u8 in match order; n_inliers [P] i64, or -1 where the host
 * estimator returns -1 -- there R, t and the pair's mask are 0.
 * Stream-ordered on `stream`; the matches never leave the device.  The call copies the per-hypothesis inlier counts to the host once,
 * replays the RANSAC loop there (the host estimator's own pow / log), copies one decision per pair back and waits for the stream
 * before it returns: two host round trips per batch, whatever P.  Workspace:
 * loftr_estimate_absolute_pose_batched_workspace_bytes(M, P), about 430 kB per pair plus 65 bytes per match.
 * Status: LOFTR_ERR_BAD_ARG for a null pointer, M < 0 or P < 0, P == 0 with M > 0, and for m_bids outside [0, P) or not grouped by
 * ascending pair (found on the device, reported at the call's own synchronisation; the outputs are then not written);
 * LOFTR_ERR_WORKSPACE for a short workspace; LOFTR_ERR_UNSUPPORTED for M >= 2^31 or P >= 2^31 / 1000.
 * M == 0 is valid (every pair gets -1); P == 0 and M == 0 is a no-op success. */
size_t loftr_estimate_absolute_pose_batched_workspace_bytes(long M, int P);
int loftr_estimate_absolute_pose_batched(const float* pts3d, const float* kpts, const long* m_bids, long M, const float* K, int P,
                                         float thresh_px, float conf, unsigned seed, float* R_out, float* t_out, uint8_t* inliers_out,
                                         long* n_inliers, void* ws, size_t ws_bytes, void* stream);

/* Matched keypoints of the image that has a depth map -> 3D points: the first half of the reference's warp_kpts
 * (src/loftr/utils/geometry.py:22-37), fp32 as there, a thread per match (csrc/absolute_pose_gpu.hip).  Device memory, stream-ordered.
 *   kpts [M,2] pixels of the depth map's image, m_bids [M] i64 pair ids, depth [P,dh,dw] f32, K [P,3,3] f32 upper triangular,
 *   T [P,4,4] f32 camera-to-world or NULL.
 * The depth is read at the keypoint rounded half to even (rintf, = torch.round); valid = the rounded keypoint lies inside the map and
 * that depth != 0.  X = K^-1 (x d, y d, d) with the UNROUNDED keypoint and the closed-form inverse
 * (Y = (y d - cy d) / fy, X = (x d - skew Y - cx d) / fx, Z = d), then X <- T[:3,:3] X + T[:3,3] when T is given; every product and
 * sum is rounded on its own (no fused multiply-add), left to right.
 * Outputs: pts3d_out [M,3] f32, valid_out [M] u8.  Invalid rows are (0, 0, 0): a keypoint outside the map (or not a number) and a pair
 * id outside [0, P) are invalid, never clamped, and no depth is read for them.  Nearest lookup only (no bilinear interpolation).
 * Status: LOFTR_ERR_BAD_ARG for a null pointer, negative sizes or P == 0 with M > 0; M == 0 is a no-op success. */
int loftr_lift_keypoints(const float* kpts, const long* m_bids, long M, const float* depth, int dh, int dw, const float* K, const float* T,
                         int P, float* pts3d_out, uint8_t* valid_out, void* stream);

/* ---- keypoint atlas: pair-list matches -> consolidated keypoints, index matches, tracks ------------------------------
 * LoFTR has no detector: every pair yields fresh sub-pixel points.  The atlas snaps the matched points of each image to a grid of
 * cell_px cells, keeps one keypoint per occupied cell, rewrites every row's matches as keypoint index pairs (one-to-one per row) and
 * links them into tracks -- the step between the pair-list driver and any multi-view consumer.  All of it is integer and order-defined:
 * loftr_atlas_host (csrc/atlas.hip, plain C++ on host arrays) DEFINES the result, loftr_atlas_observe + loftr_atlas_finalize
 * (csrc/atlas_gpu.hip) reproduce it bit for bit, whatever the arrival order of the atomics.
 *   Rule 1: cell = ((int)floorf(x * inv), (int)floorf(y * inv)), inv = fp32(1) / fp32(cell_px) computed by the caller, on a gw x gh grid per
 *     image.  A match is dropped for the FIRST of these reasons (counts[4 + reason]; 0 = valid): 1 its m_bids entry is outside [0, n);
 *     2 its mask byte is 0; 3 a coordinate or its confidence is not finite; 4 its confidence is negative; 5 a cell lies outside the grid.
 *     Dropped matches contribute nothing (neither of their two observations is used).
 *   Rule 2: one keypoint per (image, cell) with an observation: position and score of the observation with the greatest confidence, ties
 *     to the smallest observation index (2 m + side, m the match index in arrival order); n_obs = observations in the cell; keypoints
 *     ordered by image, then row-major by cell.
 *   Rule 3: a match (k_a, k_b) is kept when, on each side, it is the best (greatest confidence, then smallest match index) among its ROW's
 *     valid matches that share its keypoint on that side.  Kept matches stay in input order; matches hold LOCAL keypoint indices.
 *   Rule 4: tracks = connected components over the kept matches; label = smallest global keypoint index; components of at least
 *     min_track_len keypoints are numbered by ascending label; track_ok = no two keypoints of the component in one image.
 * The rows of one observe call must come in ascending m_bids order (as the matcher emits them), so that matches are grouped by row.
 * Limits (LOFTR_ERR_UNSUPPORTED beyond): M <= 2^31 - 2 matches, n_images * gh * gw < 2^31 cells, R <= 2^30 rows, gw, gh <= 2^24.
 *
 * Outputs (host memory for loftr_atlas_host, device memory for loftr_atlas_finalize), sized by the bound Kb = min(2 M, n_images gh gw):
 *   kp_offsets [n_images+1] i64, keypoints [Kb,2] f32, score [Kb] f32, n_obs [Kb] i32, row_offsets [R+1] i64, matches [M,2] i32,
 *   match_conf [M] f32, track_id [Kb] i32 (-1: none), track_len [Kb] i32, track_ok [Kb] u8, counts [16] i64:
 *   counts[0] = K keypoints, [1] = Mk kept matches, [2] = T tracks, [3] = status bits of the observe calls (1: an m_bids entry out of
 *   range, 2: m_bids not ascending), [4 + reason] = matches per reason.  Only the first K / Mk / T entries are written. */
typedef struct {
  long* kp_offsets; float* keypoints; float* score; int* n_obs;
  long* row_offsets; int* matches; float* match_conf;
  int* track_id; int* track_len; uint8_t* track_ok; long* counts;
} LoftrAtlasOut;

/* The defining host routine.  kpts0 / kpts1 [M,2] f32, conf [M] f32, rows [M] i32 global row of each match in ascending order, mask [M] u8
 * or NULL, row_images [R,2] i32 (image of side 0 / side 1 of every row; a != b, both in [0, n_images)).
 * Status: LOFTR_ERR_BAD_ARG for null pointers, negative sizes, rows out of [0, R) or not ascending, bad row_images; M == 0 and R == 0 succeed. */
int loftr_atlas_host(const float* kpts0, const float* kpts1, const float* conf, const int* rows, const uint8_t* mask, long M,
                     const int* row_images, long R, int n_images, int gh, int gw, float inv, int min_track_len, const LoftrAtlasOut* out);

/* Observe (what KeypointAtlas.add runs; stream-ordered, never waits): one thread per match of the chunk.  Match i of the chunk is global
 * match match_base + i and belongs to row row_base + m_bids[i]; its record (obs_xy [2 cap,2] f32, obs_cell [2 cap] i32 global cell or -1,
 * m_conf [cap] f32, m_row [cap] i32, m_reason [cap] u8; cap >= match_base + n) is stored and each valid observation issues one 64-bit
 * atomicMax into grid [n_images * gh * gw] u64 (zero before the first call).  row_images [>= row_base + n_rows, 2] i32 device,
 * status [1] i32 device (zero before the first call; bits as counts[3]).  n == 0 is a no-op success. */
int loftr_atlas_observe(const float* kpts0, const float* kpts1, const float* conf, const long* m_bids, const uint8_t* mask, long n,
                        int n_rows, long match_base, long row_base, const int* row_images, int n_images, int gh, int gw, float inv,
                        unsigned long long* grid, float* obs_xy, int* obs_cell, float* m_conf, int* m_row, uint8_t* m_reason, int* status,
                        void* stream);

/* Finalize: compact the grid into keypoints (the grid words become keypoint indices: one finalize per atlas), resolve the matches, apply
 * the mutual-best rule through one open-addressing table (64-bit atomicCAS claims, 64-bit atomicMax reduces), union-find the kept edges,
 * number the tracks.  Stream-ordered, no host synchronisation unless stage_ms is given: the caller reads counts back once and trims.
 * stage_ms: NULL, or LOFTR_ATLAS_STAGES host floats that receive the GPU time of each stage (events; the call then waits for the stream):
 * 0 compact, 1 resolve, 2 mutual best, 3 write matches, 4 union-find, 5 labels + lengths, 6 number tracks.
 * Workspace: loftr_atlas_finalize_workspace_bytes(M, n_images, gh, gw): the table's 64 to 128 bytes per match (16 bytes per slot, a power of two of at least 4 M slots) plus 30 more. */
#define LOFTR_ATLAS_STAGES 7
size_t loftr_atlas_finalize_workspace_bytes(long M, int n_images, int gh, int gw);
int loftr_atlas_finalize(unsigned long long* grid, const float* obs_xy, const int* obs_cell, const float* m_conf, const int* m_row,
                         const uint8_t* m_reason, long M, long R, int n_images, int gh, int gw, int min_track_len, const int* status,
                         const LoftrAtlasOut* out, void* ws, size_t ws_bytes, float* stage_ms, void* stream);

/* ---- triangulation of tracks from known camera poses (csrc/triangulate_core.h holds all the arithmetic) -----------------
 * From the tracks of an atlas plus database poses to one 3D point per track: what hloc / COLMAP's point triangulator is used for before
 * localisation against an SfM model.  loftr_triangulate_tracks_host (csrc/triangulate.hip, host memory) DEFINES the result,
 * loftr_triangulate_tracks (csrc/triangulate_gpu.hip, device memory) reproduces it bit for bit, whatever `group` is.
 * Input: tracks in CSR form -- offsets [T+1] i64 (0 first, N last, ascending), obs_image [N] i32 in [0, n_images), obs_xy [N,2] f32
 *   pixels; K [n_images,3,3] f64 (only fx, skew, cx, fy, cy are read), T_cam_from_world [n_images,4,4] f64 (the top 3 x 4; R is taken as
 *   orthonormal and not checked); thresh_px; cos_min_angle = cos(minimum triangulation angle), computed by the caller.
 * Arithmetic: fp64 without FMA contraction, + - * / sqrt only.
 * Per image (24 doubles): P = K [R | t], centre c = -R^T t, M = R^T K^-1 (K^-1 by back substitution).  A camera is INVALID when an
 *   entry read, or an entry of its table, is not finite, or fx or fy is 0.
 * Per track with observations 0 .. L-1 in CSR order:
 *   1. rays: d_i = M_i (u, v, 1), normalised.
 *   2. hypothesis pairs, no random numbers: for s = 1 .. L/2 and, inside, i = 0 .. L-1 (only to L/2 - 1 when 2 s = L) the pair
 *      (i, (i + s) mod L); the enumeration stops after 64 pairs (every pair for L <= 11; loftr_triangulation_pairs exposes it).
 *   3. hypothesis h from pair (i, j): the midpoint of the two rays.  w = c_i - c_j, a = d_i.d_i, b = d_i.d_j, c = d_j.d_j, d = d_i.w,
 *      e = d_j.w, den = a c - b^2; rejected if den <= 1e-12 a c, if b / sqrt(a c) > cos_min_angle, or if s = (b e - c d) / den <= 0 or
 *      t = (a e - b d) / den <= 0 (two observations of one image reject themselves here);
 *      X = ((c_i + s d_i) + (c_j + t d_j)) / 2.  A NaN in any comparison rejects.
 *   4. observation k is an inlier iff p = P_k (X, 1) has p_z > 0 and its squared pixel distance is <= thresh_px^2; a hypothesis whose
 *      own two observations are not both inliers is discarded.
 *   5. best = greatest inlier count, then smallest h: one unsigned 64-bit maximum of count << 32 | (0xFFFFFFFF - h), 0 = none.
 *   6. refit: five Gauss-Newton steps (three unknowns) on the pixel reprojection error over the inliers of the current point; J^T J and
 *      J^T r summed sequentially in ascending observation order (p_z <= 0 adds nothing); 3 x 3 elimination in a fixed order without
 *      pivoting; a non-positive pivot or a non-finite step fails the fit and keeps the point.  A fit is adopted when it keeps at least
 *      as many inliers and repeated on the adopted point's inliers while the count strictly grows, at most 4 fits.
 *   7. tri_cos = the smallest cosine between X - c_i and X - c_j over the pairs of step 2 whose two observations are final inliers (a
 *      pair with a zero-length ray is skipped); status small_angle when tri_cos > cos_min_angle or no such pair exists.
 * Output per track: xyz [T,3] f32 (the fp64 point rounded once; NaN unless status is ok), n_inliers [T] i32 and rms_px [T] f32 (root
 *   mean squared pixel error over the final inliers) and tri_cos [T] f32 (0 / NaN / NaN unless ok or small_angle; tri_cos NaN without
 *   a pair), status [T] u8: 0 ok, 1 too_short (L < 2), 2 no_hypothesis, 3 small_angle, 4 bad_camera (L >= 2 and the track touches an
 *   invalid camera).  Per observation: obs_inlier [N] u8, zero for tracks that are not ok.
 *   counts [8] i64: [0..4] tracks per status, [5] error bits found on the device (1: an obs_image outside [0, n_images), 2: offsets
 *   that do not start at 0, end at N and ascend), [6] inlier observations of the ok tracks, [7] 0.
 * Status: LOFTR_ERR_BAD_ARG for null pointers, negative sizes, thresh_px < 0, cos_min_angle outside [-1, 1], group outside {0, 8, 64};
 *   the host routine also for bad obs_image / offsets (the kernels raise counts[5] instead: they never wait for the device, and no
 *   output is defined then); LOFTR_ERR_UNSUPPORTED for T or N >= 2^31; LOFTR_ERR_WORKSPACE for a short workspace. */
int loftr_triangulate_tracks_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, long N, const double* K,
                                  const double* T_cam_from_world, int n_images, double thresh_px, double cos_min_angle, float* xyz,
                                  int* n_inliers, float* rms_px, float* tri_cos, uint8_t* status, uint8_t* obs_inlier, long* counts);
/* The pairs of step 2 for a track of L observations: pairs [64,2] (the first *n rows written), *n = min(64, L (L - 1) / 2). */
int loftr_triangulation_pairs(int L, int* pairs, int* n);
/* The kernels.  group: 0 = a group of 8 lanes per track of at most 64 observations and of 64 lanes per longer track (two launches over
 * all tracks; the boundary is a measured tuning constant), 8 / 64 = that group size for every track (one launch); the result does not depend on it.  Stream-ordered, no host
 * synchronisation unless stage_ms is given: NULL, or LOFTR_TRIANGULATE_STAGES host floats that receive the GPU time (events; the call
 * then waits for the stream) of 0 the camera table, 1 the 8-lane launch, 2 the 64-lane launch.
 * Workspace: loftr_triangulate_tracks_workspace_bytes(T, N, n_images), the camera table (192 bytes per image); 0 for sizes out of range. */
#define LOFTR_TRIANGULATE_STAGES 3
size_t loftr_triangulate_tracks_workspace_bytes(long T, long N, int n_images);
int loftr_triangulate_tracks(const long* offsets, long T, const int* obs_image, const float* obs_xy, long N, const double* K,
                             const double* T_cam_from_world, int n_images, double thresh_px, double cos_min_angle, float* xyz,
                             int* n_inliers, float* rms_px, float* tri_cos, uint8_t* status, uint8_t* obs_inlier, long* counts, int group,
                             void* ws, size_t ws_bytes, float* stage_ms, void* stream);

/* ---- localisation against a triangulated model: query matches -> fused 2D-3D correspondences ---------------------------
 * The link between the atlas + triangulation and loftr_estimate_absolute_pose_batched: a query image is matched against several
 * database images of the model; every database-side match point is looked up among the atlas keypoints of that image, its 3D point
 * fetched, and the rows of one query merged so that no 3D point is used twice.  All of it is integer and order-defined:
 * loftr_model_lookup_host (csrc/model_lookup.hip, host memory) DEFINES the result, loftr_model_lookup (csrc/model_lookup_gpu.hip,
 * device memory) reproduces it bit for bit, whatever the arrival order of the atomics.  csrc/model_lookup_core.h holds what they share.
 * Model (built once): kp_offsets [n_images+1] i64 (0 first, K last, ascending); kp_cell [K] i32, the cell cy * gw + cx of every
 *   keypoint's stored position under rule 1 of the atlas (strictly ascending within an image: loftr_model_cells computes and checks it);
 *   kp_point [K] i32, the row of xyz of the keypoint or -1; xyz [P,3] f32; inv, gh, gw as for the atlas.
 * Queries: kpts_db / kpts_q [M,2] f32 (the match's point in the database image / in the query image), conf [M] f32, rows [M] i32
 *   ascending, mask [M] u8 or NULL, row_db [R] i32 (database image of every row), row_query [R] i32 (query of every row, in [0, Q),
 *   non-decreasing: the rows of a query are contiguous).
 *   Rule 1: a match gets the FIRST reason that applies (match_reason; counts[4 + reason]): 1 bad row (an error, below); 2 its mask byte
 *     is 0; 3 a coordinate of either point or its confidence is not finite; 4 its confidence is negative (-0.0 is not); 5 the cell of
 *     the database point lies outside the grid (the query point needs no grid); 6 no_keypoint: no keypoint of image row_db[row] has that
 *     cell (the search never leaves kp_offsets[d] .. kp_offsets[d+1]); 7 no_point: kp_point is -1 (an entry >= P, which a checked model
 *     does not have, counts the same and is never used as an index).  Anything else is a candidate of (query, point).
 *   Rule 2: of the candidates of one (query, point) the one with the greatest confidence, then the smallest match index, is kept
 *     (reason 0; one unsigned 64-bit max of conf_bits << 32 | (0xFFFFFFFF - m)), the others are fused (reason 8).  Two candidates that
 *     share a query point but reach different 3D points are both kept.
 *   Rule 3: the C kept correspondences in ascending match index (so grouped by ascending query): pts3d [C,3] f32 copies of xyz rows,
 *     kpts [C,2] f32 the query points unchanged, q_ids [C] i64, match [C] i32, point [C] i32, conf [C] f32; q_offsets [Q+1] i64;
 *     match_reason [M] u8; counts [16] i64: [0] = C, [3] = status bits, [4 + reason] = matches per reason (they sum to M under status 0).
 *     Outputs are sized by the bound C <= M; only the first C entries are written.
 *   Rule 4, status bits: 1 a rows entry outside [0, R); 2 rows descending; 4 a row_query entry outside [0, Q) or descending; 8 a row_db
 *     entry outside [0, n_images).  The host routine returns LOFTR_ERR_BAD_ARG; the kernels raise the bit in counts[3], read nothing
 *     through the bad value and leave the other outputs undefined: they never wait for the device.
 * Limits (LOFTR_ERR_UNSUPPORTED beyond, answered before a data pointer is read): M <= 2^31 - 2; Q, P, R < 2^31; K, gh * gw < 2^31;
 *   gw, gh <= 2^24.  Status: LOFTR_ERR_BAD_ARG for null pointers, negative sizes and (host routines) kp_offsets that do not start at 0,
 *   end at K and ascend; LOFTR_ERR_WORKSPACE for a short workspace; M == 0, R == 0 and Q == 0 succeed. */
typedef struct {
  const long* kp_offsets; const int* kp_cell; const int* kp_point; const float* xyz;
  long K, P;
  int n_images, gh, gw;
  float inv;
} LoftrModel;
typedef struct {
  float* pts3d; float* kpts; long* q_ids; int* match; int* point; float* conf;
  long* q_offsets; uint8_t* match_reason; long* counts;
} LoftrModelLookupOut;

/* kp_cell [K] of keypoints [K,2] f32, and *status (one int32; host memory for the host form, device memory for the kernel, which
 * zeroes it first and never waits): bit 16 when a keypoint lies outside the grid (or is not finite) or the cells do not ascend strictly
 * within an image, bit 32 when a kp_point entry leaves [-1, P). */
int loftr_model_cells_host(const long* kp_offsets, int n_images, const float* keypoints, const int* kp_point, long K, long P, int gh, int gw,
                           float inv, int* kp_cell, int* status);
int loftr_model_cells(const long* kp_offsets, int n_images, const float* keypoints, const int* kp_point, long K, long P, int gh, int gw,
                      float inv, int* kp_cell, int* status, void* stream);

/* The defining host routine (every pointer, those inside *model too, is host memory). */
int loftr_model_lookup_host(const LoftrModel* model, const float* kpts_db, const float* kpts_q, const float* conf, const int* rows,
                            const uint8_t* mask, long M, const int* row_db, const int* row_query, long R, long Q,
                            const LoftrModelLookupOut* out);
/* The kernels (*model and *out are host structs of device pointers): lookup (a thread per match and per row; table of 16-byte slots, a
 * power of two of at least 2 M, claimed by 64-bit atomicCAS and reduced by 64-bit atomicMax), keep (the table's winners; counts per
 * block and per query), two u32 scans, write.  Stream-ordered, no data-dependent grid and no host synchronisation unless stage_ms is
 * given: NULL, or LOFTR_MODEL_LOOKUP_STAGES host floats that receive the GPU time (events; the call then waits for the stream) of
 * 0 lookup (with the clearing of the table), 1 keep + scans, 2 write.  The caller reads counts back once and trims.
 * Workspace: loftr_model_lookup_workspace_bytes(M, Q): the table's 32 to 64 bytes per match, 8 more per match, 4 per query; 0 for
 * sizes out of range. */
#define LOFTR_MODEL_LOOKUP_STAGES 3
size_t loftr_model_lookup_workspace_bytes(long M, long Q);
int loftr_model_lookup(const LoftrModel* model, const float* kpts_db, const float* kpts_q, const float* conf, const int* rows,
                       const uint8_t* mask, long M, const int* row_db, const int* row_query, long R, long Q, const LoftrModelLookupOut* out,
                       void* ws, size_t ws_bytes, float* stage_ms, void* stream);

/* ---- bundle adjustment of the triangulated model (csrc/bundle_core.h holds all the arithmetic and every per-item step) ------
 * Joint refinement of camera poses (6 DoF, intrinsics fixed) and points over the pixel reprojection error: Levenberg-Marquardt, optional
 * Huber loss, the point-eliminated Schur system solved by preconditioned conjugate gradients without forming it.
 * loftr_bundle_adjust_host (csrc/bundle.hip, host memory) DEFINES the result, loftr_bundle_adjust (csrc/bundle_gpu.hip, device memory)
 * reproduces it bit for bit, whatever the grid.
 * Input: tracks in CSR form as for the triangulation -- offsets [T+1] i64, obs_image [N] i32, obs_xy [N,2] f32 -- plus obs_mask [N] u8,
 *   xyz [T,3] f32, K [n,3,3] f64 (fx, skew, cx, fy, cy read), T_cam_from_world [n,4,4] f64, fixed [n] u8, and the observations grouped by
 *   image: cam_offsets [n+1] i64 (0 first, N last, ascending), cam_obs [N] i32, the observation indices of image 0, then of image 1, ...,
 *   strictly ascending within an image (the stable sort of obs_image).
 * Arithmetic: fp64 without FMA contraction, + - * / sqrt only.
 *   1. State.  A camera is a unit quaternion (w, x, y, z) and t.  The quaternion comes from the input R by Shepperd's method, branch on
 *      the largest of trace, R00, R11, R22 (the first of equals), then divided by its norm.  A camera is VALID when fx, skew, cx, fy, cy,
 *      the top 3 x 4 of its matrix and its quaternion are finite and fx, fy are not 0.  The rotation used for a valid camera that is not
 *      fixed is R(q); for any other camera it is the input's R.  Points are fp64 copies of the f32 xyz.  A camera that is not free gets
 *      its 16 input doubles back bit for bit, a point that is not active its 3 input floats.
 *   2. Active set, fixed for the run.  An observation is active iff its mask byte is non-zero, its pixel is finite, its camera is valid,
 *      its point is finite and Y_z > 0 at the start; a point with fewer than 2 such observations is inactive and so are its
 *      observations.  A camera is free iff it is not fixed, valid, and has at least 1 active observation.
 *   3. P = R X, Y = P + t, u = fx (Y0 / Y2) + skew (Y1 / Y2) + cx, v = fy (Y1 / Y2) + cy, r = (u, v) - obs.  With the perturbation
 *      Y' = dR P + t + dt: A = dr/d(omega, dt) [2,6] with dY/domega = -[P]x, B = dr/dX = (dr/dY) R [2,3].
 *   4. Huber: |r| = sqrt(ru^2 + rv^2); w = 1, rho = |r|^2 if huber_px is 0 or |r| <= huber_px, else w = huber_px / |r|,
 *      rho = 2 huber_px |r| - huber_px^2.  A, B and r enter the normal equations multiplied by sqrt(w); the cost is the sum of rho.
 *   5. Sums.  Per point (V = sum B^T B, g = sum B^T r, its shares of the cost and of sum |r|^2): sequentially over the track's active
 *      observations in CSR order.  Per camera (U = sum A^T A, 21 entries; g_c = sum A^T r; the camera half of S p): osum64 over the
 *      camera's list, element l being slot l of the list (an inactive slot adds nothing).  osum64: 64 accumulators start at +0;
 *      accumulator l adds elements l, l + 64, ... ascending; then for s = 32, 16, ..., 1: a[l] = a[l] + a[l + s] for l < s; the result is
 *      a[0].  osum (the cost over tracks, dot products over cameras): osum64 per chunk of 4096 elements, then osum of the chunk sums.
 *      A dot product of camera vectors is 6 terms sequentially per camera (+0 for a camera that is not free), then osum over cameras.
 *   6. Step.  The diagonals of U and V are multiplied by 1 + lambda (a zero diagonal becomes lambda).  V^-1 and the block-Jacobi
 *      preconditioner U^-1 are L D L^T eliminations in index order without pivoting; a non-positive pivot rejects the step.  Right-hand
 *      side b = -(g_c - sum A^T (B y_j)), y_j = V^-1 g_j.  S x = b by preconditioned conjugate gradients from x = 0 over the free
 *      cameras; S p is evaluated as z_j = V^-1 sum B^T (A p_c) per point (over its active observations of free cameras), then
 *      U p_c - sum A^T (B z_j) per camera.  Before each of the at most pcg_iters iterations the solve stops when
 *      r.M^-1 r <= pcg_tol^2 r0.M^-1 r0, and after S p when p.S p is not greater than 0.  Points: dX_j = V^-1 (-(g_j + sum B^T (A x_c))).
 *      With no free camera this is the per-point step.
 *   7. Trial: q' = normalise((1, omega / 2) (x) q), t' = t + dt, X' = X + dX; a non-finite value rejects.  Accepted iff every active
 *      observation keeps Y_z > 0 and cost' < cost; then lambda = max(lambda / 10, 1e-10), and the run stops as converged when
 *      cost - cost' <= ftol cost'.  Rejected: lambda = 10 lambda, and the run stops as stalled when lambda > 1e10.  lambda starts at 1e-4;
 *      A, B, U, V are evaluated again only after an accepted trial.  At most max_iters trials; none when there is no active observation
 *      (status 3) or when the cost of the start is exactly 0 (converged).
 * Output: T_out [n,4,4] f64 (R(q), t and the row 0 0 0 1 for a free camera), xyz_out [T,3] f32 (the fp64 point rounded once),
 *   obs_active [N] u8, cam_free [n] u8, point_active [T] u8, counts [16] i64: [0] status -- 0 converged, 1 max_iters, 2 stalled,
 *   3 nothing to adjust (no active observation) --, [1] error bits (1: an obs_image outside [0, n); 2: offsets that do not start at 0,
 *   end at N and ascend; 4: cam_offsets / cam_obs that are not the stable grouping), [2] trials, [3] accepted trials, [4] conjugate
 *   gradient iterations, [5] active observations, [6] active points, [7] free cameras, [8..12] the bits of five doubles: cost before,
 *   cost after, rms pixel error over the active observations before and after, final lambda; [13..15] 0.
 * Status: LOFTR_ERR_BAD_ARG for null pointers, negative sizes, huber_px or ftol negative or not finite, pcg_tol outside [0, 1),
 *   max_iters outside [0, LOFTR_BUNDLE_MAX_ITERS], pcg_iters outside [1, LOFTR_BUNDLE_MAX_PCG]; the host routine also for the three
 *   error bits (the kernels raise counts[1] instead, read nothing through the bad value, run no trial and leave the other outputs
 *   undefined: they never wait for the device); LOFTR_ERR_UNSUPPORTED for T or N >= 2^31; LOFTR_ERR_WORKSPACE for a short workspace. */
#define LOFTR_BUNDLE_MAX_ITERS 1000
#define LOFTR_BUNDLE_MAX_PCG 200
int loftr_bundle_adjust_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                             const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed, int n_images,
                             const long* cam_offsets, const int* cam_obs, double huber_px, int max_iters, int pcg_iters, double pcg_tol,
                             double ftol, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free, uint8_t* point_active,
                             long* counts);
/* The kernels: a fixed schedule of launches on the stream (max_iters trials of pcg_iters iterations); a kernel whose phase the host
 * routine would not run returns at once on a flag in device memory.  No host synchronisation unless class_ms is given: NULL, or
 * 2 * LOFTR_BUNDLE_CLASSES host floats that receive, per kernel class, the median GPU time of a launch and the total (events around
 * every launch; the call then waits for the stream).  class_launches: NULL, or LOFTR_BUNDLE_CLASSES host longs, the launches issued.
 * Classes: 0 setup, 1 linearise, 2 factor, 3 track half, 4 camera half, 5 osum, 6 update, 7 apply, 8 evaluate, 9 accept, 10 write.
 * Workspace: loftr_bundle_adjust_workspace_bytes(T, N, n_images): 208 bytes per track, 4 per observation, about 960 per image; 0 for
 * sizes out of range. */
#define LOFTR_BUNDLE_CLASSES 11
size_t loftr_bundle_adjust_workspace_bytes(long T, long N, int n_images);
int loftr_bundle_adjust(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                        const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed, int n_images,
                        const long* cam_offsets, const int* cam_obs, double huber_px, int max_iters, int pcg_iters, double pcg_tol,
                        double ftol, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free, uint8_t* point_active,
                        long* counts, void* ws, size_t ws_bytes, float* class_ms, long* class_launches, void* stream);

/* ---- bundle adjustment with per-image focal refinement -------------------------------------------------------------------
 * The rule above with a camera block of 7 parameters instead of 6; everything not named here is that rule unchanged.
 * loftr_bundle_adjust_focal_host DEFINES the result, loftr_bundle_adjust_focal reproduces it bit for bit.
 *   Parameter.  One scalar per camera, a relative focal step delta: the trial is fx' = fx (1 + delta), skew' = skew (1 + delta),
 *      fy' = fy (1 + delta); cx and cy stay fixed.
 *   Jacobian.  The seventh column of A is sqrt(w) (fx a + skew b, fy b) with a = Y0 / Y2, b = Y1 / Y2, evaluated from the current
 *      state's intrinsics like the other six columns; + - * / sqrt only, fp64, contraction off.
 *   Which cameras.  Camera i REFINES ITS FOCAL iff it is free (rule 2), refine_focal[i] != 0 and it has at least min_focal_obs (>= 1)
 *      active observations.  Any other camera has a zero seventh column, so its delta is exactly 0, and its K comes back bit for bit.
 *      A fixed camera refines nothing.
 *   Block sizes.  Camera blocks are 7 x 7: U has 28 entries, g_c has 7, a dot product of camera vectors has 7 terms, sequential; the
 *      camera osum64 of the linearisation carries 35 accumulators per lane.  Sums, tree orders and flags are rule 5's.
 *   Bounds.  focal_lo < 1 < focal_hi, finite.  A trial is rejected, like a non-finite value in rule 7, when for a refining camera fx'
 *      or fy' is not finite, or fx' / fx_in or fy' / fy_in is not strictly inside (focal_lo, focal_hi) (fx_in, fy_in: the input K's).
 * Input added: refine_focal [n] u8, min_focal_obs, focal_lo, focal_hi.  Output added: K_out [n,3,3] f64 (the input's bits for a camera
 *   that does not refine; else fx, skew, cx, fy, cy of the final state and the other four entries copied), cam_focal [n] u8, and
 *   counts[13] = the number of refining cameras.
 * Status: as above; LOFTR_ERR_BAD_ARG also for min_focal_obs < 1, bounds that are not finite or do not straddle 1, and null
 *   refine_focal / K_out / cam_focal with n_images > 0.  Workspace: loftr_bundle_adjust_focal_workspace_bytes (about 1100 bytes per image).
 * Out of scope: principal point, focal refinement of a fixed-pose camera (the grouped rule below has it), focal priors.
 *   PARITY UNPINNED against Ceres / COLMAP. */
int loftr_bundle_adjust_focal_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                                   const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                   const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs, double huber_px,
                                   int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs, double focal_lo,
                                   double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free,
                                   uint8_t* point_active, double* K_out, uint8_t* cam_focal, long* counts);
size_t loftr_bundle_adjust_focal_workspace_bytes(long T, long N, int n_images);
int loftr_bundle_adjust_focal(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                              const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                              const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs, double huber_px,
                              int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs, double focal_lo, double focal_hi,
                              double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free, uint8_t* point_active, double* K_out,
                              uint8_t* cam_focal, long* counts, void* ws, size_t ws_bytes, float* class_ms, long* class_launches,
                              void* stream);

/* ---- bundle adjustment with one focal step per GROUP of images (one physical camera) --------------------------------------
 * The two rules above with ONE relative focal step delta_g per group of images instead of one per image; everything not named here is
 * unchanged.  loftr_bundle_adjust_shared_host DEFINES the result, loftr_bundle_adjust_shared reproduces it bit for bit.
 *   Groups.  cam_group [n] i32 (the group of image i, in [0, G)), group_offsets [G+1] i64 (0 first, n last, ascending, no empty group),
 *      group_cams [n] i32: the members of group 0, then of group 1, ..., strictly ascending within a group, the groups in the order of
 *      their first members (the stable sort of cam_group after that relabelling).  1 <= G <= n (G = 0 with n = 0).
 *   Who carries.  Image i CARRIES iff it is valid, refine_focal[i] != 0 and it has at least 1 active observation; its pose may be fixed.
 *      Group g REFINES iff its carrying members together have at least min_focal_obs active observations.  cam_focal[i] = i carries and
 *      its group refines.  A member without cam_focal gets its K back bit for bit.  What is shared is the step, not the value: every
 *      member with cam_focal takes fx' = fx (1 + delta_g), skew' = skew (1 + delta_g), fy' = fy (1 + delta_g) on its own fx, skew, fy.
 *      The products are formed through the group: s_g starts at 1, a trial has s_g' = s_g (1 + delta_g), and the member's trial values
 *      are fx_in s_g', skew_in s_g', fy_in s_g' (the input K's), so that after any number of accepted trials the members of a group
 *      differ from their inputs by ONE factor, each rounded once.
 *   Live cameras.  A camera takes part in the step when it is free or has cam_focal.  The six pose columns of A are +0 for a camera that is
 *      not free (`fixed` speaks of the pose only here), the seventh is +0 for one without cam_focal.  U (28 entries) and g_c (7) are summed
 *      for every live camera by rule 5's osum64.  A camera that is not free gets its 16 pose doubles back bit for bit.
 *   Operator.  With S7, b7 the 7-wide quantities of §18.1 and E copying delta_g into the seventh slot of the members with cam_focal, the
 *      system is E^T S7 E x = E^T b7 over 6 unknowns per free camera and 1 per refining group.  E^T: osum64 over the group's list, element
 *      l being the l-th member; a member without cam_focal adds nothing.  The point half is rule 6's over the active observations of live
 *      cameras, the vector of a camera being (its 6 pose entries, or +0 when it is not free; its group's entry, or +0 without cam_focal).
 *      The camera half of a free camera is rows 0..5 of U7d p - sum A^T (B z_j), U7d with its first six diagonals damped.  The seventh
 *      entry of a member with cam_focal is sum_{k<6} U_k7 p_k - (sum A^T (B z_j))_7; the group's entry is d p_g + E^T of those, where
 *      d_g = E^T of U77 and d = d_g (1 + lambda), or lambda when d_g is 0: damped once, at the group.  The right-hand side is
 *      E^T of b7 = -(g_c - sum A^T (B y_j)) likewise.
 *   Preconditioner.  The 6 x 6 L D L^T of the damped pose block per free camera, and 1 / d per refining group.  A non-positive pivot or a
 *      non-positive d rejects the step.
 *   Dot products.  6 terms sequentially per camera (+0 when it is not free), osum over the cameras; 1 term per group (+0 when it does
 *      not refine), osum over the groups; the result is the camera sum plus the group sum, in that order.
 *   Trial.  Rule 7 for the free cameras; the focal step and §18.1's bound test for every member with cam_focal.
 * Input added to §18.1's: cam_group, group_offsets, group_cams, G.  Output added: group_focal [G] u8; counts[13] = the images with
 *   cam_focal, counts[14] = the refining groups.  Error bit 8 of counts[1]: cam_group / group_offsets / group_cams are not that grouping
 *   (the host routine returns LOFTR_ERR_BAD_ARG, the kernels raise the bit, read nothing through the bad value and run no trial).
 * Status: §18.1's; LOFTR_ERR_BAD_ARG also for G outside [1, n] (0 with n = 0) and null group arrays.  Workspace:
 *   loftr_bundle_adjust_shared_workspace_bytes: §18.1's plus 76 bytes per image (sized by n_images, whatever G is).
 * Out of scope: groups that share a value rather than a step, principal point, focal priors (one radial coefficient per group: the
 *   rule after the next).  PARITY UNPINNED. */
int loftr_bundle_adjust_shared_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                                    const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                    const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                    const int* cam_group, const long* group_offsets, const int* group_cams, int G, double huber_px,
                                    int max_iters, int pcg_iters, double pcg_tol, double ftol, int min_focal_obs, double focal_lo,
                                    double focal_hi, double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free,
                                    uint8_t* point_active, double* K_out, uint8_t* cam_focal, uint8_t* group_focal, long* counts);
size_t loftr_bundle_adjust_shared_workspace_bytes(long T, long N, int n_images);
int loftr_bundle_adjust_shared(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                               const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                               const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs, const int* cam_group,
                               const long* group_offsets, const int* group_cams, int G, double huber_px, int max_iters, int pcg_iters,
                               double pcg_tol, double ftol, int min_focal_obs, double focal_lo, double focal_hi, double* T_out,
                               float* xyz_out, uint8_t* obs_active, uint8_t* cam_free, uint8_t* point_active, double* K_out,
                               uint8_t* cam_focal, uint8_t* group_focal, long* counts, void* ws, size_t ws_bytes, float* class_ms,
                               long* class_launches, void* stream);

/* ---- bundle adjustment with position priors on the camera centres (GPS) ----------------------------------------------------
 * Any of the three rules above (mode 0: §18, 1: §18.1, 2: §18.2) with one more term per camera: its centre is held near a measured
 * position.  Everything not named here is the rule of its mode unchanged; fp64 without contraction, + - * / sqrt only.
 * loftr_bundle_adjust_prior_host DEFINES the result, loftr_bundle_adjust_prior reproduces it bit for bit.  A prior couples no point, so
 * the point elimination, S p, the preconditioner and the conjugate gradients are untouched: only U, g_c and the cost of a camera change.
 *   Input added.  prior_xyz [n,3] f64 (world units), prior_sigma [n,3] f64 (per axis, world units), prior_mask [n] u8.
 *   Which cameras.  Camera i HAS A PRIOR iff it is free (rule 2), prior_mask[i] != 0, its three positions are finite and its three
 *      sigmas are finite and > 0 (a NaN deactivates).  A camera that is not free -- a fixed-pose member of a group included -- never has
 *      one: its term would be a constant.  cam_prior [n] u8 records the decision.
 *   Residual.  c_k = -((R_0k t_0 + R_1k t_1) + R_2k t_2) (c = -R^T t, R and t of the state), d_k = c_k - g_k, e_k = d_k / sigma_ik.
 *   Jacobian.  With §18's perturbation R' = dR R, t' = t + dt: dc/d omega = -R^T [t]x, dc/d dt = -R^T.  Row k, with r = column k of R:
 *      J_k = (-(r_1 t_2 - r_2 t_1), -(r_2 t_0 - r_0 t_2), -(r_0 t_1 - r_1 t_0), -r_0, -r_1, -r_2), each entry divided by sigma_ik.
 *      3 x 6; the focal column of the 7-wide modes is not touched.
 *   Sums.  After the camera's osum64 over its observations: U_ab += (J_0a J_0b + J_1a J_1b) + J_2a J_2b for a <= b < 6 and
 *      g_c,a += (J_0a e_0 + J_1a e_1) + J_2a e_2 for a < 6, one addition per entry.  A camera without a prior performs no addition.
 *   Cost.  cost = osum(track shares) + osum(camera shares), one addition, tracks first; a camera's share is (e_0^2 + e_1^2) + e_2^2, +0
 *      without a prior.  A second camera osum carries (d_0^2 + d_1^2) + d_2^2 for the report.  rms_px and sum |r|^2 stay over the
 *      observations.  The prior's loss is the square: huber_px acts on the observations only (remove gross errors through prior_mask).
 *   Trial, acceptance and stopping are rule 7 on the combined cost; "nothing to adjust" is decided by the active observations alone.
 * Arguments: those of loftr_bundle_adjust_shared(_host), then the prior inputs and mode after G, and cam_prior before counts.  The focal
 *   arguments are ignored and may be NULL with mode 0, the group arguments with mode < 2.
 * counts [24] i64: 0..15 as in the mode; 16 = cameras with a prior; 17, 18 = bits of the prior cost (the cameras' osum, in sigma^2)
 *   before and after; 19, 20 = bits of the root mean squared |c - g| over the cameras with a prior, before and after (world units, 0
 *   without any); 21..23 = 0.
 * Status: the mode's; LOFTR_ERR_BAD_ARG also for mode outside 0..2 and for NULL prior_xyz / prior_sigma / prior_mask / cam_prior with
 *   n_images > 0.  The error bits are unchanged.  Workspace: loftr_bundle_adjust_prior_workspace_bytes(T, N, n_images, mode): the mode's
 *   plus 16 bytes per image; 0 for sizes out of range or a mode outside 0..2.
 * Out of scope: rotation priors, priors on points, a robust prior loss, lever arms, covariances with off-diagonal terms.  PARITY UNPINNED. */
int loftr_bundle_adjust_prior_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                                   const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                   const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                   const int* cam_group, const long* group_offsets, const int* group_cams, int G, const double* prior_xyz,
                                   const double* prior_sigma, const uint8_t* prior_mask, int mode, double huber_px, int max_iters,
                                   int pcg_iters, double pcg_tol, double ftol, int min_focal_obs, double focal_lo, double focal_hi,
                                   double* T_out, float* xyz_out, uint8_t* obs_active, uint8_t* cam_free, uint8_t* point_active,
                                   double* K_out, uint8_t* cam_focal, uint8_t* group_focal, uint8_t* cam_prior, long* counts);
size_t loftr_bundle_adjust_prior_workspace_bytes(long T, long N, int n_images, int mode);
int loftr_bundle_adjust_prior(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                              const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                              const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs, const int* cam_group,
                              const long* group_offsets, const int* group_cams, int G, const double* prior_xyz, const double* prior_sigma,
                              const uint8_t* prior_mask, int mode, double huber_px, int max_iters, int pcg_iters, double pcg_tol,
                              double ftol, int min_focal_obs, double focal_lo, double focal_hi, double* T_out, float* xyz_out,
                              uint8_t* obs_active, uint8_t* cam_free, uint8_t* point_active, double* K_out, uint8_t* cam_focal,
                              uint8_t* group_focal, uint8_t* cam_prior, long* counts, void* ws, size_t ws_bytes, float* class_ms,
                              long* class_launches, void* stream);

/* ---- bundle adjustment with one radial coefficient per GROUP of images ----------------------------------------------------
 * The grouped rule (§18.2) with the camera model x_d = x (1 + k r^2), y_d = y (1 + k r^2) on normalised coordinates and ONE additive
 * step dk_g of k per group next to its relative focal step; everything not named here is §18.2's: fp64 without contraction, + - * /
 * sqrt only, the active set decided once, the Huber loss, the orders of the sums, the flags, the error bits.
 * loftr_bundle_adjust_radial_host DEFINES the result, loftr_bundle_adjust_radial reproduces it bit for bit.  Only this rule reads a k.
 *   Input added to §18.2's: radial_in [n] f64 (the start values), refine_radial [n] u8, radial_lo <= radial_hi (finite).
 *   Projection, in this order: a = Y0 / Y2, b = Y1 / Y2, r2 = a a + b b, m = 1 + k r2, xd = a m, yd = b m,
 *      r = (((fx xd + skew yd) + cx) - u, (fy yd + cy) - v).  Evaluate, the track linearisation and the track half read it.
 *   Jacobians.  jaa = m + 2k (a a), jab = 2k (a b), jbb = m + 2k (b b) (d(xd, yd)/d(a, b) = m I + 2k (a, b)(a, b)^T);
 *      ua = fx jaa + skew jab, ub = fx jab + skew jbb, va = fy jab, vb = fy jbb; du = sw (ua / Y2, ub / Y2, -((ua a + ub b) / Y2)),
 *      dv likewise from va, vb.  The pose columns of A and B are rule 3's products of du, dv (the v row has no zero entry here).
 *      Column 7 (focal) = sw (fx xd + skew yd, fy yd) with cam_focal, column 8 (radial) = sw (fx (a r2) + skew (b r2), fy (b r2))
 *      with cam_radial, +0 otherwise.  U has 36 entries, g_c 8.
 *   Who carries.  A valid image whose radial_in is not finite is not valid.  cam_focal and group_focal are §18.2's.  Image i is a radial
 *      candidate iff it carries (§18.2) and refine_radial[i] != 0; group g REFINES ITS RADIAL iff it refines its focal and its candidates
 *      together have at least min_focal_obs active observations (group_radial [G]); cam_radial[i] = i is a candidate and its group does.
 *   Group block.  2 unknowns per refining group, focal first.  D_g = (U77, U78; U78, U88) summed over the members with cam_focal by
 *      osum64 over the member list.  Each diagonal is damped once, at the group: d (1 + lambda), or lambda when d is 0; a group that
 *      does not refine its radial has U78 = U88 = +0 and right-hand side +0 there.  Preconditioner: the 2 x 2 L D L^T of the damped
 *      block in rule 6's fixed order; a non-positive pivot rejects the step.  E^T: the seventh entries of the members with cam_focal
 *      and the eighth of those with cam_radial, osum64 each; the rows U_k7, U_k8 (k < 6) of a member enter its seventh and eighth
 *      entry as U_k7 does in §18.2.  Group entry: Sp_0 = (d_00 p_0 + d_01 p_1) + E^T_0, Sp_1 = (d_01 p_0 + d_11 p_1) + E^T_1.
 *   Dot products.  The cameras' osum (6 terms each), then the groups' (2 terms each, focal first), added in that order.
 *   Trial.  a_g starts at +0; a trial has a_g' = a_g + dk_g and every member with cam_radial k' = radial_in + a_g' (one rounding on the
 *      input whatever the number of accepted trials).  A k' outside [radial_lo, radial_hi] (a NaN fails) rejects the trial, like a
 *      focal outside its bounds.
 *   Output added: radial [n] f64 (the input's bits for an image without cam_radial), cam_radial [n] u8, group_radial [G] u8;
 *      counts[15] = the images with cam_radial.
 * Status: §18.2's; LOFTR_ERR_BAD_ARG also for null radial arrays with n_images > 0 and bounds that are not finite or not ordered.
 * Workspace: loftr_bundle_adjust_radial_workspace_bytes (sized by n_images, whatever G is).
 * Out of scope: per-image 8 x 8 blocks, priors together with radial, refining k with a trusted focal, k2, tangential and fisheye
 *   terms, principal point.  PARITY UNPINNED. */
int loftr_bundle_adjust_radial_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                                    const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                                    const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs,
                                    const int* cam_group, const long* group_offsets, const int* group_cams, int G, const double* radial_in,
                                    const uint8_t* refine_radial, double huber_px, int max_iters, int pcg_iters, double pcg_tol, double ftol,
                                    int min_focal_obs, double focal_lo, double focal_hi, double radial_lo, double radial_hi, double* T_out,
                                    float* xyz_out, uint8_t* obs_active, uint8_t* cam_free, uint8_t* point_active, double* K_out,
                                    uint8_t* cam_focal, uint8_t* group_focal, double* radial_out, uint8_t* cam_radial,
                                    uint8_t* group_radial, long* counts);
size_t loftr_bundle_adjust_radial_workspace_bytes(long T, long N, int n_images);
int loftr_bundle_adjust_radial(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                               const float* xyz, const double* K, const double* T_cam_from_world, const uint8_t* fixed,
                               const uint8_t* refine_focal, int n_images, const long* cam_offsets, const int* cam_obs, const int* cam_group,
                               const long* group_offsets, const int* group_cams, int G, const double* radial_in,
                               const uint8_t* refine_radial, double huber_px, int max_iters, int pcg_iters, double pcg_tol, double ftol,
                               int min_focal_obs, double focal_lo, double focal_hi, double radial_lo, double radial_hi, double* T_out,
                               float* xyz_out, uint8_t* obs_active, uint8_t* cam_free, uint8_t* point_active, double* K_out,
                               uint8_t* cam_focal, uint8_t* group_focal, double* radial_out, uint8_t* cam_radial, uint8_t* group_radial,
                               long* counts, void* ws, size_t ws_bytes, float* class_ms, long* class_launches, void* stream);

/* ---- pixels without the radial coefficient (csrc/radial_core.h holds the arithmetic) ------------------------------------------
 * Every stage but the adjustment above reads pinhole pixels; this gives them.  xy [M,2] f32, image [M] i32, K [n,9] f64, radial [n] f64
 * -> xy_out [M,2] f32, ok [M] u8, counts [8] i64.  One fp64 text for both sides, a point depends on its own inputs only.
 * loftr_undistort_points_host DEFINES the result, loftr_undistort_points (a thread per point) reproduces it bit for bit.
 *   1. y_d = (v - cy) / fy, x_d = ((u - cx) - skew y_d) / fx, r_d = sqrt(x_d^2 + y_d^2).
 *   2. r = r_d, then 12 times r = r - (r (1 + k (r r)) - r_d) / (1 + 3k (r r)): a FIXED count, no data-dependent exit.
 *   3. ok iff fx, skew, cx, fy, cy, k, u, v, r_d and r are finite, fx and fy are not 0, 1 + 3k (r r) > 0 at the result and
 *      |r (1 + k (r r)) - r_d| <= 1e-9 (1 + r_d).
 *   4. m = 1 + k (r r); the output is ((fx (x_d / m) + skew (y_d / m)) + cx, fy (y_d / m) + cy) rounded to f32, and must be finite;
 *      a point that is not ok is (NaN, NaN) with ok = 0 (the triangulation rejects pixels that are not finite).
 *   k = 0 is ok and the point is recomputed through K: NOT promised to be the input's bits.
 * counts: 0 = points ok, 1 = error bits, 2 = points not ok, 3..7 = 0.  Error bit 1: an image outside [0, n_images); the host routine
 *   returns LOFTR_ERR_BAD_ARG, the kernels raise the bit, and neither writes anything beyond the counts.
 * loftr_distort_points_host is the other direction from the same text (m = 1 + k (x x + y y), (x m, y m) through K), for the tests
 *   and the tools.  LOFTR_ERR_BAD_ARG: negative sizes, null arrays that would be read or written. */
int loftr_undistort_points_host(const float* xy, const int* image, long M, const double* K, const double* radial, int n_images,
                                float* xy_out, uint8_t* ok, long* counts);
int loftr_undistort_points(const float* xy, const int* image, long M, const double* K, const double* radial, int n_images, float* xy_out,
                           uint8_t* ok, long* counts, void* stream);
int loftr_distort_points_host(const float* xy, const int* image, long M, const double* K, const double* radial, int n_images,
                              float* xy_out, uint8_t* ok, long* counts);

/* ---- correspondence table of the images without a pose (csrc/register_core.h holds every per-item step) -------------------
 * The 2D-3D correspondences that the tracks give the images that have no pose yet, gathered per image in a defined order: the input of
 * one batched absolute-pose call (loftr_estimate_absolute_pose_batched) that registers them.  Integer work and bit copies only.
 * loftr_register_corr_host (csrc/register.hip, host memory) DEFINES the result, loftr_register_corr (csrc/register_gpu.hip, device
 * memory) reproduces it bit for bit.
 * Input: tracks in CSR form as for the bundle adjustment -- offsets [T+1] i64, obs_image [N] i32, obs_xy [N,2] f32 --, xyz [T,3] f32 and
 *   status [T] u8 of the triangulation (0 = ok), posed [n] u8, the observations grouped by image -- cam_offsets [n+1] i64, cam_obs [N] i32,
 *   the stable sort of obs_image, checked here as there -- and min_corr >= 4.
 *   1. Observation o of track j is a correspondence iff posed[obs_image[o]] == 0, status[j] == 0, the three floats of xyz[j] are finite
 *      and the two floats of obs_xy[o] are finite (NaN fails).
 *   2. n_corr[i] = the correspondences in image i's list; 0 for a posed image.
 *   3. Image i is a candidate iff it is not posed and n_corr[i] >= min_corr.  Candidates are numbered in ascending image id:
 *      cand_rank [n] i32 (-1 otherwise), cand_image [P] i32.
 *   4. The table holds the correspondences of the candidates only: candidates in ascending rank, within a candidate the order of its
 *      cam_obs list (ascending observation index).  corr_xyz [C,3] f32 and corr_xy [C,2] f32 are bit copies, corr_bid [C] i64 is the rank,
 *      corr_obs [C] i32 the observation index, cand_offsets [P+1] i64 the candidates' row ranges.
 *   5. counts [8] i64: [0] C, [1] P, [2] error bits (1: an obs_image outside [0, n); 2: offsets that do not start at 0, end at N and
 *      ascend; 4: cam_offsets / cam_obs that are not the stable grouping), [3] unposed images, [4] unposed images with at least one
 *      correspondence, [5] correspondences including those of non-candidates, [6] the largest n_corr, [7] 0.
 * Output buffers are sized by the bounds: n_corr, cand_rank, cand_image [n]; cand_offsets [n+1]; corr_* [N] rows; rows past P / C are
 *   not written.
 * Status: LOFTR_ERR_BAD_ARG for null pointers, negative sizes, min_corr < 4, observations without a track or an image; the host
 *   routine also for the three error bits (the kernels raise counts[2] instead, read nothing through the bad value, write C = P = 0 and
 *   nothing else); LOFTR_ERR_UNSUPPORTED for T or N >= 2^31; LOFTR_ERR_WORKSPACE for a short workspace. */
int loftr_register_corr_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, long N, const float* xyz,
                             const uint8_t* status, const uint8_t* posed, int n_images, const long* cam_offsets, const int* cam_obs,
                             int min_corr, int* n_corr, int* cand_rank, int* cand_image, long* cand_offsets, float* corr_xyz, float* corr_xy,
                             long* corr_bid, int* corr_obs, long* counts);
/* The kernels: four launches on the stream (0 flags per track, 1 counts per image, 2 ranks and offsets -- one workgroup that walks the
 * images in blocks of LOFTR_REGISTER_RANK_BLOCK --, 3 rows per candidate).  No host synchronisation unless stage_ms is given: NULL, or
 * LOFTR_REGISTER_STAGES host floats that receive the GPU time of each launch (the call then waits for the stream).
 * Workspace: loftr_register_corr_workspace_bytes(T, N, n_images): 5 bytes per observation, 4 per image; 0 for sizes out of range. */
#define LOFTR_REGISTER_STAGES 4
#define LOFTR_REGISTER_RANK_BLOCK 256
size_t loftr_register_corr_workspace_bytes(long T, long N, int n_images);
int loftr_register_corr(const long* offsets, long T, const int* obs_image, const float* obs_xy, long N, const float* xyz,
                        const uint8_t* status, const uint8_t* posed, int n_images, const long* cam_offsets, const int* cam_obs,
                        int min_corr, int* n_corr, int* cand_rank, int* cand_image, long* cand_offsets, float* corr_xyz, float* corr_xy,
                        long* corr_bid, int* corr_obs, long* counts, void* ws, size_t ws_bytes, float* stage_ms, void* stream);

/* ---- track completion: points claim the atlas keypoints they project onto (csrc/complete_core.h holds every per-item step) --
 * The atlas makes a track only where matches of different rows snapped to the same cell, so one physical point tends to end as several
 * short tracks and loose keypoints.  Completion projects every row that has a 3D point into every posed image the row does not visit
 * and lets it claim the nearest free keypoint there; its whole result is a relabelled kp_row (the atlas's track_id).
 * loftr_complete_tracks_host (csrc/complete.hip, host memory) DEFINES the result, loftr_complete_tracks (csrc/complete_gpu.hip, device
 * memory) reproduces it bit for bit.
 * Input: the CSR of the rows a triangulation ran on -- offsets [T+1] i64, obs_image [N] i32 --, its xyz [T,3] f32 and status [T] u8
 *   (0 = ok); the keypoint pool -- kp_offsets [n+1] i64, keypoints [K,2] f32, kp_cell [K] i32 (cy * gw + cx, strictly ascending within
 *   an image, as loftr_model_cells makes and checks it), kp_row [K] i32 (the row that holds the keypoint, or -1) --; K [n,9] and
 *   T_cam_from_world [n,16] f64, from which the camera table of the triangulation is built (P = K [R | t]; an invalid camera is all
 *   NaN); posed [n] u8; the grid (inv, gh, gw) of the atlas; thresh_px (thr2 = thresh_px * thresh_px in fp64); reach in
 *   [0, LOFTR_COMPLETE_MAX_REACH] cells.  Arithmetic: fp64 without FMA contraction, + - * / only.
 *   1. Source.  Row j is a source iff status[j] == 0 and the three floats of xyz[j] are finite (exponent bits not all ones).
 *   2. Target.  Image i is a target of j iff posed[i] != 0, its camera is valid, and no observation of row j lies in image i.
 *      obs_image must not descend within a row (the routines merge-walk it).
 *   3. Projection.  X = (double) xyz[j]; x = (P0 . X) + P03, y = (P1 . X) + P13, z = (P2 . X) + P23 with (a0 b0 + a1 b1) + a2 b2 as the
 *      dot product (the triangulation's residual); z > 0 is required; u = x / z, v = y / z; cx = floorf((float) u * inv) if that lies in
 *      [0, gw), cy likewise from v and gh; otherwise the pair has no candidates.
 *   4. Candidates.  The keypoints of image i whose cell (cy', cx') has |cy' - cy| <= reach and |cx' - cx| <= reach, clipped to the grid:
 *      for each cell row in ascending order one lower-bound search of cy' gw + max(cx - reach, 0) in kp_cell over
 *      [kp_offsets[i], kp_offsets[i+1]), then a walk while the cell is at most cy' gw + min(cx + reach, gw - 1).  Keypoint k is WITHIN iff
 *      r2(k) = (x / z - kx)^2 + (y / z - ky)^2 <= thr2 (NaN fails); it is FREE iff kp_row[k] == -1 or status[kp_row[k]] != 0: a row
 *      without a point yields its keypoints, a row with a point never does.
 *   5. Proposal.  The proposal of (j, i) is the free keypoint within the threshold with the smallest (bits of (float) r2, k).  A pair
 *      makes at most one proposal: a row never gains two keypoints in one image, nor one in an image it already visits.
 *   6. Winner.  A keypoint proposed by several rows goes to the smallest ((uint64) bits of (float) r2 << 32) | j: one unsigned 64-bit
 *      minimum.  A row that loses gets nothing in that image; there is no second choice.
 *   7. Output.  kp_row_new [K] i32: the winner's row where there was one, kp_row[k] elsewhere; link_r2 [K] f32: the winner's (float) r2,
 *      NaN elsewhere; counts [8] i64: [0] accepted links, [1] error bits, [2] sources, [3] (source, target) pairs, [4] pairs in front
 *      and inside the grid, [5] proposals, [6] proposals that lost, [7] pairs without a proposal that have a keypoint within the
 *      threshold owned by a row WITH a point (what track merging, below, serves).
 *   8. Errors (counts[1]).  1: an obs_image outside [0, n); 2: offsets (kp_offsets) that do not start at 0, end at N (K) and ascend;
 *      4: obs_image descending within a row; 8: a kp_row outside [-1, T).
 * Status: LOFTR_ERR_BAD_ARG for null pointers, negative sizes, thresh_px negative or not finite, reach out of range, observations
 *   without a row, keypoints without an image; the host routine also for the four error bits, and it then writes the bits to counts[1] and nothing else (the kernels
 *   raise counts[1] instead, read nothing through the bad value, and write counts[0] = 0, kp_row_new = kp_row, link_r2 = NaN);
 *   LOFTR_ERR_UNSUPPORTED for T or N >= 2^31, K > 2^31 - 1, a grid beyond the atlas's limits, more than 65535 image chunks;
 *   LOFTR_ERR_WORKSPACE for a short workspace.
 * Out of scope: merging two rows that both have a point, descriptor or fine-level verification of a link, second choices, changing the
 *   two-view matches, per-image extents.  PARITY UNPINNED against COLMAP's CompleteTracks. */
#define LOFTR_COMPLETE_MAX_REACH 8
int loftr_complete_tracks_host(const long* offsets, long T, const int* obs_image, long N, const float* xyz, const uint8_t* status,
                               const long* kp_offsets, const float* keypoints, const int* kp_cell, const int* kp_row, long K,
                               const double* Kmat, const double* T_cam_from_world, const uint8_t* posed, int n_images, float inv, int gh,
                               int gw, double thresh_px, int reach, int* kp_row_new, float* link_r2, long* counts);
/* The kernels: two memsets (the claims, the counts) and four launches on the stream (0 the camera table, 1 the checks, 2 the links -- a
 * thread per row and LOFTR_COMPLETE_IMAGE_CHUNK images per blockIdx.y; a proposal is one 64-bit atomic minimum --, 3 a thread per
 * keypoint that writes the output).  No host synchronisation unless stage_ms is given: NULL, or LOFTR_COMPLETE_STAGES host floats that
 * receive the GPU time of each launch (the call then waits for the stream).
 * Workspace: loftr_complete_tracks_workspace_bytes(T, N, K, n_images): 192 bytes per image, 8 per keypoint; 0 for sizes out of range. */
#define LOFTR_COMPLETE_STAGES 4
#define LOFTR_COMPLETE_IMAGE_CHUNK 64
size_t loftr_complete_tracks_workspace_bytes(long T, long N, long K, int n_images);
int loftr_complete_tracks(const long* offsets, long T, const int* obs_image, long N, const float* xyz, const uint8_t* status,
                          const long* kp_offsets, const float* keypoints, const int* kp_cell, const int* kp_row, long K,
                          const double* Kmat, const double* T_cam_from_world, const uint8_t* posed, int n_images, float inv, int gh, int gw,
                          double thresh_px, int reach, int* kp_row_new, float* link_r2, long* counts, void* ws, size_t ws_bytes,
                          float* stage_ms, void* stream);

/* ---- track merging: rows whose points meet and agree become one track (csrc/merge_core.h holds every per-item step) ---------
 * Completion stops where two rows both have a point.  Merging serves those meetings: a row with a point that projects onto a keypoint
 * held by another row with a point, in an image it does not visit, becomes one row with it when the two share no image and every
 * defining observation of both agrees with their weighted point.  Its whole result is again a relabelled kp_row.
 * loftr_merge_tracks_host (csrc/merge.hip, host memory) DEFINES the result, loftr_merge_tracks (csrc/merge_gpu.hip, device memory)
 * reproduces it bit for bit.
 * Input: everything loftr_complete_tracks_host takes, plus obs_xy [N,2] f32 (the pixel of every observation) and obs_mask [N] u8 (the
 *   observations that define the row's point: the triangulation's obs_inlier).  Arithmetic: fp64 without FMA contraction, + - * / only;
 *   thr2 = thresh_px * thresh_px.
 *   1. Source.  Row j is a source as in completion (status[j] == 0, finite xyz); w[j] = the number of its observations with
 *      obs_mask != 0.
 *   2. Meeting.  A source row j is projected into every target image i (posed, valid camera, not visited by j) by completion's rules
 *      2-4: the same projection, cells and visiting order.  Its candidate in i is the keypoint k with r2(k) <= thr2 and the smallest
 *      (bits of (float) r2, k) among those whose kp_row[k] = m is ANOTHER source row (m >= 0, m != j, m a source).  Free keypoints and
 *      keypoints of rows without a point are ignored.  A (row, image) pair makes at most one meeting (j, m).
 *   3. Disjoint.  The meeting is compatible iff rows j and m share no image: a merge walk over the two ascending obs_image lists, over
 *      all observations, masked or not.  A merged track therefore never visits an image twice.
 *   4. Agreement.  a = min(j, m), b = max(j, m); rejected if w[a] == 0 or w[b] == 0;
 *      X[c] = ((double) w[a] * Xa[c] + (double) w[b] * Xb[c]) / (double)(w[a] + w[b]) in this operation order; every masked observation
 *      of both rows must lie in an image that is posed with a valid camera and satisfy residual2(camera, X, obs_xy) <= thr2 (in front;
 *      NaN fails).  The pair's score is the largest of these r2, held as the bits of (float) r2.  It depends on (a, b) alone.
 *   5. Choice.  best [T] u64 starts as all ones (the empty entry).  An accepted meeting (j, m) does two unsigned 64-bit minima:
 *      (bits << 32) | m into best[j], (bits << 32) | j into best[m].  For a fixed row the order by (bits, partner) is the order of its
 *      pairs by (bits, min, max), a total order on pairs, so the globally smallest accepted pair is always mutual.
 *   6. Merge.  Rows j and m merge iff each is the other's best.  The lower row survives: row_into[j] = row_into[m] = min(j, m);
 *      row_into[t] = t elsewhere.  merge_r2[t] = the pair's score as a float for both rows of a merged pair, NaN elsewhere.  One pass:
 *      a row merges with at most one other row, there are no chains; a call after a new triangulation merges further.
 *   7. Output.  row_into [T] i32, merge_r2 [T] f32, kp_row_new [K] i32 = kp_row[k] < 0 ? kp_row[k] : row_into[kp_row[k]];
 *      counts [8] i64: [0] merged pairs, [1] error bits, [2] sources, [3] (source, target) pairs, [4] meetings, [5] disjoint meetings,
 *      [6] accepted meetings, [7] relabelled keypoints.  A pair met in several images or from both sides counts once per meeting;
 *      every count is defined by the rule, none depends on a schedule.
 *   8. Errors (counts[1]).  Completion's four bits with the same behaviour.
 * Status: as loftr_complete_tracks_host; the host routine returns LOFTR_ERR_BAD_ARG for the four error bits after writing them to
 *   counts[1] and nothing else; the kernels raise counts[1] instead, read nothing through the bad value and write row_into = identity,
 *   merge_r2 = NaN, kp_row_new = kp_row, counts[0] = 0.
 * Out of scope: chains and multi-way merges in one pass, merging through shared images, re-estimating the point (the next
 *   triangulation does), descriptor checks, changing the two-view matches.  PARITY UNPINNED against COLMAP's MergeTracks. */
int loftr_merge_tracks_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                            const float* xyz, const uint8_t* status, const long* kp_offsets, const float* keypoints, const int* kp_cell,
                            const int* kp_row, long K, const double* Kmat, const double* T_cam_from_world, const uint8_t* posed,
                            int n_images, float inv, int gh, int gw, double thresh_px, int reach, int* row_into, float* merge_r2,
                            int* kp_row_new, long* counts);
/* The kernels: two memsets (best, the counts) and five launches on the stream (0 the camera table and 1 the checks, completion's; 2 the
 * meetings -- a thread per row and LOFTR_MERGE_IMAGE_CHUNK images per blockIdx.y; an accepted meeting is two 64-bit atomic minima --,
 * 3 a thread per row that writes row_into and merge_r2, 4 a thread per keypoint that writes kp_row_new).  No host synchronisation unless
 * stage_ms is given: NULL, or LOFTR_MERGE_STAGES host floats that receive the GPU time of each launch (the call then waits for the
 * stream).  Workspace: loftr_merge_tracks_workspace_bytes(T, N, K, n_images): 192 bytes per image, 8 per row; 0 for sizes out of range. */
#define LOFTR_MERGE_STAGES 5
#define LOFTR_MERGE_IMAGE_CHUNK 64
size_t loftr_merge_tracks_workspace_bytes(long T, long N, long K, int n_images);
int loftr_merge_tracks(const long* offsets, long T, const int* obs_image, const float* obs_xy, const uint8_t* obs_mask, long N,
                       const float* xyz, const uint8_t* status, const long* kp_offsets, const float* keypoints, const int* kp_cell,
                       const int* kp_row, long K, const double* Kmat, const double* T_cam_from_world, const uint8_t* posed, int n_images,
                       float inv, int gh, int gw, double thresh_px, int reach, int* row_into, float* merge_r2, int* kp_row_new, long* counts,
                       void* ws, size_t ws_bytes, float* stage_ms, void* stream);

/* ---- track splitting: consistent tracks from the components that visit an image twice (csrc/split_core.h holds every
 * per-item step) -----------------------------------------------------------------------------------------------------------------------
 * Rule 4 of the atlas makes a track of every connected component of the kept matches and marks it track_ok = 0 when two of its keypoints
 * lie in one image; every consumer then drops it whole.  Splitting grows the keypoints of such a track again along its matches,
 * strongest first, never joining two components that share an image.  Integer and order-defined, one unsigned 64-bit maximum per
 * decision.  loftr_split_tracks_host (csrc/split.hip, host memory) DEFINES the result, loftr_split_tracks (csrc/split_gpu.hip, device
 * memory) reproduces it bit for bit.
 * Input: edge_kp [E,2] i32 (the kept matches as GLOBAL keypoint indices; edge e is match e), edge_conf [E] f32, kp_image [K] i32 (must
 *   not descend: keypoints are ordered by image), track_id [K] i32 (-1: none), track_ok [T] u8, n_images, min_track_len >= 1,
 *   max_rounds >= 0.
 *   1. Open edges.  Edge e = (u, v) is OPEN iff track_id[u] == track_id[v] = t >= 0 and track_ok[t] == 0; every other edge is IGNORED.
 *   2. Frozen and free keypoints.  A keypoint of a track with track_ok != 0 is frozen: its label is the smallest keypoint index of its
 *      track.  A keypoint with track_id = -1 has no label.  A keypoint of a track with track_ok == 0 is free and starts as a component
 *      of its own: label = its index, member list = itself.  A member list ascends by keypoint index, so by image.
 *   3. Round r = 0 .. max_rounds - 1, three phases over the open edges; no phase reads what it writes.
 *      propose: label[u] == label[v] makes the edge INTERNAL.  Otherwise the two member lists are walked in step; an image that occurs
 *        in both (two endpoints in one image included) makes the edge CONFLICT, for good, because components only grow.  Otherwise the
 *        edge is a candidate with the word (bits of edge_conf[e], -0.0 as +0.0) << 32 | (0xFFFFFFFF - e), and best[label[u]] and
 *        best[label[v]] take the maximum of the word (best starts every round as 0).
 *      accept: a candidate whose word equals both best entries is accepted.  Words are unique, so a component is in at most one accepted
 *        edge of a round; the greatest candidate is always accepted.
 *      merge: for every accepted edge the two lists are spliced into one ascending list, every member takes the smaller label (the head
 *        of a list is its label), and the edge becomes INTERNAL.  round_accepted[r] = the accepted edges.  A round that accepts nothing
 *        ends the procedure.
 *   4. An edge that is still a candidate after the last round stays OPEN: counts[5] > 0 means max_rounds was too small to finish (a
 *      chain whose confidences descend merges one edge per round).
 *   5. Numbering, as rule 4 of the atlas over frozen and grown components together: the labels with at least min_track_len members, in
 *      ascending label, are the tracks 0 .. T' - 1; track_id_new [K] i32 (-1 elsewhere), track_len_new [K] i32 (the first T' entries;
 *      0 behind them).  Every numbered track visits an image at most once.
 *   6. edge_state [E] u8: 0 ignored, 1 internal, 2 conflict, 3 open.  round_accepted [max_rounds] i32.  counts [16] i64: [0] T',
 *      [1] error bits, [2..5] ignored / internal / conflict / open edges, [6] tracks with track_ok == 0, [7] their keypoints, [8] those
 *      of them that end in a numbered track, [9] rounds that accepted something, [10] the members of the largest grown component,
 *      the rest 0.
 *   7. Errors (counts[1]).  1: an edge_kp entry outside [0, K); 2: a track_id outside [-1, T) or a kp_image outside [0, n_images);
 *      4: kp_image descends; 8: an edge_conf that is not finite or is negative; 16: a member list longer than n_images, which no valid
 *      input produces and which bounds every walk: n_images + 1 steps on either list.
 * Status: LOFTR_ERR_BAD_ARG for null pointers, negative sizes, min_track_len < 1; the host routine also for the error bits, and it then
 *   writes the bits to counts[1] and nothing else (the kernels raise counts[1] instead, read nothing through the bad value and write
 *   no other output); LOFTR_ERR_UNSUPPORTED for E > 2^31 - 2, K or T >= 2^31, max_rounds >= 2^20; LOFTR_ERR_WORKSPACE.
 * Out of scope: geometric verification (the triangulation's inlier test follows), a second home for the keypoints that end -1
 *   (completion may claim them), any criterion but the match confidence, a sequential greedy (Kruskal) order, the atlas's rule 4. */
int loftr_split_tracks_host(const int* edge_kp, const float* edge_conf, long E, const int* kp_image, const int* track_id, long K,
                            const uint8_t* track_ok, long T, int n_images, int min_track_len, int max_rounds, int* track_id_new,
                            int* track_len_new, uint8_t* edge_state, int* round_accepted, long* counts);
/* The kernels: memsets, a check and an init launch, per round a memset of best and three launches (propose and accept a thread per edge,
 * merge a thread per accepted edge), then lengths, flags, the u32 scan, numbering and one launch that writes the outputs.  A round's
 * launches return at once when counts[1] is set or the round before accepted nothing.  No host synchronisation unless stage_ms is
 * given: NULL, or LOFTR_SPLIT_STAGES(max_rounds) host floats (check + init; per round: clear, propose, accept, merge; number; write; the
 * call then waits for the stream).  Workspace: loftr_split_tracks_workspace_bytes(E, K, T, max_rounds): 24 bytes per keypoint, 5 per
 * edge, 4 per track and per round; 0 for sizes out of range. */
#define LOFTR_SPLIT_STAGES(max_rounds) (3 + 4 * (max_rounds))
size_t loftr_split_tracks_workspace_bytes(long E, long K, long T, int max_rounds);
int loftr_split_tracks(const int* edge_kp, const float* edge_conf, long E, const int* kp_image, const int* track_id, long K,
                       const uint8_t* track_ok, long T, int n_images, int min_track_len, int max_rounds, int* track_id_new,
                       int* track_len_new, uint8_t* edge_state, int* round_accepted, long* counts, void* ws, size_t ws_bytes,
                       float* stage_ms, void* stream);

/* ---- track refinement: the fine stage at points the caller names (csrc/refine_core.h holds the per-row step) ------------
 * The atlas snaps matched points to cells, so the observations of a track are up to one cell apart.  Refinement re-localises every
 * observation of a track against one reference view with the matcher's fine level.  What that needs of the library is narrow: every
 * other entry point places the fine windows at coarse cells chosen by coarse matching; these two place them at given points.
 * Side 0 is the reference (its point is snapped to the fine grid and fixed), side 1 the query (refined, as loftr_fine_match refines it).
 *
 * loftr_refine_centres_host (csrc/refine.hip, host memory) DEFINES the result, loftr_refine_centres (csrc/refine_gpu.hip, device
 * memory, a thread per row, one launch, no synchronisation) reproduces it bit for bit.
 *   pts0, pts1 [M,2] f32 (x, y) in the coordinates the forward returns; b_ids [M] i64 the pair of every row; scale0 / scale1 NULL or
 *   [n_pairs,2] f32 (w, h) as in the batch dict; (hf, wf) the fine-map extents and (hc, wc) the coarse-map extents per side; stride =
 *   fine pixels per coarse cell; s = image pixels per fine pixel.  All arithmetic in fp32 without contraction.
 *   1. Per side and axis the centre is c = clamp((int)floorf(p / scale[b] / s + 0.5f), 0, extent - 1); without a scale the division by
 *      it is left out.  The clamp is taken on the float, so no value outside int is converted.
 *   2. The coarse cell per axis is min((c + stride / 2) / stride, extent_c - 1); i_ids / j_ids [M] i64 = cell_y * wc + cell_x.  A centre
 *      stride * cell gives back that cell.
 *   3. The snapped point per axis is (float)c * s, then * scale[b] where a scale is given: at c = stride * cell the bits of the
 *      forward's mkpts0_c / mkpts1_c.
 *   4. ok [M] u8 = 0 where a coordinate is not finite or b is outside [0, n_pairs) (no scale is read for such a row); the row then has
 *      centre 0, cell 0 and the snapped point (0, 0), so nothing downstream reads out of range.
 *   Outputs: c0, c1 [M,2] i32 (x, y) in fine pixels, i_ids, j_ids [M] i64, pts0_s, pts1_s [M,2] f32, ok [M] u8.
 * Status: LOFTR_ERR_BAD_ARG for M < 0, n_pairs < 0, an extent or stride that is not positive, s not finite or not positive, and null
 *   arrays with M > 0 (scale0 / scale1 may be NULL); M == 0 is a no-op success; LOFTR_ERR_UNSUPPORTED for M >= 2^39 on the GPU. */
int loftr_refine_centres_host(const float* pts0, const float* pts1, const int64_t* b_ids, long M, const float* scale0,
                              const float* scale1, int n_pairs, int hf0, int wf0, int hf1, int wf1, int h0c, int w0c, int h1c, int w1c,
                              int stride, float s, int* c0, int* c1, int64_t* i_ids, int64_t* j_ids, float* pts0_s, float* pts1_s,
                              uint8_t* ok);
int loftr_refine_centres(const float* pts0, const float* pts1, const int64_t* b_ids, long M, const float* scale0, const float* scale1,
                         int n_pairs, int hf0, int wf0, int hf1, int wf1, int h0c, int w0c, int h1c, int w1c, int stride, float s,
                         int* c0, int* c1, int64_t* i_ids, int64_t* j_ids, float* pts0_s, float* pts1_s, uint8_t* ok, void* stream);

/* loftr_fine_preprocess_gather with the windows at given centres: the window of match m on side 0 covers
 * [c0y - W/2, c0y + W/2] x [c0x - W/2, c0x + W/2] of bank_f0[slot0[b_ids[m]]], zero outside the map, side 1 likewise; c0, c1 [M,2] i32
 * (x, y) in fine pixels (device memory; any value is safe, a centre far outside the map gives a window of zeros).  i_ids / j_ids are
 * still what the coarse gather reads (loftr_refine_centres gives the cells that hold the centres), w0c / w1c and stride are accepted
 * and checked as in the twin and not read by the window gather.  Per-element arithmetic and store as in loftr_fine_preprocess_gather:
 * at c = stride * cell the outputs are that entry point's, bit for bit.  Everything after the window gather, the workspace
 * (loftr_fine_preprocess_workspace_bytes) and the status codes as for loftr_fine_preprocess_gather; c0 / c1 NULL with M > 0 is
 * LOFTR_ERR_BAD_ARG. */
int loftr_fine_preprocess_gather_at(const loftr_fmap* bank_f0, int n_slots0, const int32_t* slot0,
                                    const loftr_fmap* bank_f1, int n_slots1, const int32_t* slot1,
                                    const float* feat_c0, const float* feat_c1, int L, int S, int Cc,
                                    const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M,
                                    int w0c, int w1c, int stride, int W, int Cf,
                                    const float* down_w, const float* down_b, const float* merge_w,
                                    const float* merge_b, float* out0, float* out1, void* ws,
                                    size_t ws_bytes, const int* c0, const int* c1, void* stream);

/* ---- rotation averaging over the view graph; the pairs that disagree (csrc/rotation_core.h holds every per-item step) ---
 * The image pairs with their relative rotations are the edges of a graph over the images.  Relative rotations around a cycle must
 * compose to the identity, so a pair that no cycle supports is suspect; robust averaging gives one rotation per image, and every pair
 * a residual against them.  fp64, `+ - * /` and sqrt only, no contraction, every sum in a stated order.
 * loftr_rotation_averaging_host (csrc/rotation.hip, host memory) DEFINES the result, loftr_rotation_averaging (csrc/rotation_gpu.hip,
 * device memory) reproduces it bit for bit.  Rotations are unit quaternions (w, x, y, z) inside, by §18's Shepperd conversion.
 * Input: edge_image [E,2] i32 (a, b); edge_R [E,3,3] f64 with x_b = R x_a, so R_b = R_ab R_a for camera-from-world rotations;
 *   edge_weight [E] i32 (for example inlier counts); n_images; root (-1: rule 4); the adjacency the caller builds with integer
 *   sorts: adj_offsets [n_images + 1] i64 and adj_edge [2E] i32, the edges of every node ordered by (neighbour, edge); edge_use_in
 *   [E] u8 (rule 2).  Angles arrive converted: cycle_cos_half = cos(cycle / 2), loss_chord = 2 sin(loss / 2), max_chord =
 *   2 sin(max_err / 2), step_tol in radians.
 *   1. Checks (counts[1]).  1: an edge_image entry outside [0, n_images); 2: a == b; 4: adj_offsets that do not start at 0, end at 2E
 *      and ascend, a slot that does not hold an edge of its node, neighbours that descend, edges that do not ascend strictly within a
 *      neighbour, or two used edges that join one pair; 8: root outside [-1, n_images).
 *   2. Edge e is VALID iff its weight is positive, its matrix is finite, det > 0 and max |R^T R - I| <= 1e-3 (the zeros of a refused
 *      model are invalid, not an error).  Among the valid edges of one unordered pair the caller marks the heaviest (ties: the lowest
 *      index) in edge_use_in; edge_use = edge_use_in on valid edges, 0 on the others; valid edges that are not used are duplicates.
 *   3. support[e] of a used edge (a, b): the nodes c that both ends reach by a used edge and whose cycle quaternion
 *      q_ca (x) q_bc (x) q_ab (a factor conjugated when its edge is stored the other way round) has |w| >= cycle_cos_half;
 *      saturates at 65535; 0 for the other edges.
 *   4. With root = -1 the root is the image with the greatest i64 sum of used weights, the lowest on ties.  Only the root's
 *      component is solved, which need not be the largest.
 *   5. The tree is the maximum spanning forest of the used edges under the strict order of the words
 *      min(support, 0xFFFF) << 48 | min(weight, 0xFFFF) << 32 | (0xFFFFFFFF - e).  Words are unique, so the forest is: the host runs
 *      Kruskal, the kernels Boruvka rounds in which every component accepts its best outgoing edge.
 *   6. Start values: q_root = (1, 0, 0, 0); along the tree away from the root q_child = normalise(q (x) q_parent), q the edge's
 *      quaternion from the parent's side.  Images the root does not reach have in_graph = 0.
 *   7. At most max_iters Gauss-Newton steps over the used edges of the graph.  Residual of edge (a, b): e = conj(q_b) (x) q_ab (x) q_a
 *      with the sign that makes e.w >= 0, r = 2 e.xyz (the chord).  Weight w = weight (d^2 / (d^2 + |r|^2))^2, d = loss_chord
 *      (Geman-McClure); the robust cost is the osum over the edges of weight d^2 |r|^2 / (d^2 + |r|^2).  The step omega minimises
 *      sum_e w_e |r_e - (omega_b - omega_a)|^2 with omega_root = 0: Jacobi-preconditioned conjugate gradients from 0, at most pcg_iters
 *      iterations, ended by r.z <= pcg_tol^2 (r.z)_0; a node's sums run over its list in order, dot products over the 3 n_images
 *      scalars by §18's osum.  q_i <- normalise(q_i (x) (1, omega_i / 2)).  The refinement ends when the largest |omega_i| is below
 *      step_tol (status 0), after max_iters (1), or on a step that is not finite, which is not applied (2); 3: the root has no used edge.
 *   8. Every valid edge with both ends in the graph, duplicates included, gets edge_chord [E] f64 = |r| at the final state and
 *      edge_state [E] u8 = 2 (ok: chord <= max_chord) or 3 (outlier); the others have chord NaN and state 0 (invalid) or 1 (an end
 *      outside the graph).  R [n_images,3,3] f64: exactly the identity at the root, NaN outside the graph.  in_graph [n_images] u8,
 *      support [E] i32, tree [E] u8, edge_use [E] u8.  counts [16] i64: [0] images in the graph, [1] error bits, [2..4] invalid /
 *      duplicate / used edges, [5] the sum of support, [6] tree edges, [7] tree edges with support 0 (the warning sign: the tree had to
 *      cross an edge no cycle vouches for), [8] the depth of the tree below the root, [9] components of the used edges, [10] outer
 *      iterations, [11] conjugate-gradient iterations, [12] ok, [13] outlier edges, [14] status, [15] the root (-1 without images).
 *      info [4] f64: the robust cost at the start values and at the end, the last step (radians), the largest chord of an ok edge.
 * Status: LOFTR_ERR_BAD_ARG for null pointers, negative sizes, edges without images, loss_chord <= 0, a negative max_chord or step_tol,
 *   pcg_tol outside [0, 1), anything not finite; the host routine also for the error bits, and it then writes the bits to counts[1] and
 *   nothing else (the kernels raise counts[1] instead, read nothing through the bad value and write no other output);
 *   LOFTR_ERR_UNSUPPORTED for E > 2^31 - 2, n_images > 2^30, max_iters or pcg_iters > 65536; LOFTR_ERR_WORKSPACE.
 * Out of scope: translations and global positions, rotation priors for the bundle adjustment, the components the root does not reach,
 *   any weighting but the caller's integers.  The defaults of the Python layer come from synthetic graphs only. */
int loftr_rotation_averaging_host(const int* edge_image, const double* edge_R, const int* edge_weight, long E, int n_images, int root,
                                  const long* adj_offsets, const int* adj_edge, const uint8_t* edge_use_in, double cycle_cos_half,
                                  double loss_chord, double max_chord, double step_tol, int max_iters, int pcg_iters, double pcg_tol,
                                  double* R, uint8_t* in_graph, uint8_t* edge_state, double* edge_chord, int* support, uint8_t* tree,
                                  uint8_t* edge_use, long* counts, double* info);
/* The kernels: a fixed schedule of launches that depends on the sizes, max_iters and pcg_iters only; a launch whose phase the host
 * routine would not run returns at once on flags an earlier launch wrote.  No host synchronisation unless stage_ms is given: NULL, or
 * LOFTR_ROTATION_STAGES host floats (check, support, tree, start, refine, write; the call then waits for the stream).  Workspace:
 * loftr_rotation_averaging_workspace_bytes(E, n_images): about 90 bytes per edge and 190 per image; 0 without images (none is needed
 * then) and for sizes out of range. */
#define LOFTR_ROTATION_STAGES 6
size_t loftr_rotation_averaging_workspace_bytes(long E, int n_images);
int loftr_rotation_averaging(const int* edge_image, const double* edge_R, const int* edge_weight, long E, int n_images, int root,
                             const long* adj_offsets, const int* adj_edge, const uint8_t* edge_use_in, double cycle_cos_half,
                             double loss_chord, double max_chord, double step_tol, int max_iters, int pcg_iters, double pcg_tol,
                             double* R, uint8_t* in_graph, uint8_t* edge_state, double* edge_chord, int* support, uint8_t* tree,
                             uint8_t* edge_use, long* counts, double* info, void* ws, size_t ws_bytes, float* stage_ms, void* stream);

/* ---- 3D similarity between two point sets; moving a model into another frame ------------------------------------------
 * dst ~ s R src + t with R a proper rotation and s > 0, or s == 1 when with_scale == 0 (rigid, SE(3)): the closed form of Kabsch /
 * Umeyama (PAMI 1991) inside RANSAC and as the refit (csrc/similarity.hip; what georegistration against surveyed camera centres and
 * 3D-3D registration of two depth-lifted point sets need).  HOST function: all pointers are host memory, the call is synchronous.
 * src [M,3], dst [M,3] fp64; thresh and every residual are in the units of dst.
 *   Sampling: loftr_estimate_pose's own -- xorshift64* from `seed`, 3 distinct indices, at most 1000 iterations, a hypothesis replaces
 *   the best only with strictly more inliers, the adaptive stop log(1 - conf) / log(1 - w^3).  The sample stream does not depend on
 *   the scores.
 *   Solver (fp64): centroids mu_s, mu_d; H = sum (dst_i - mu_d)(src_i - mu_s)^T = U diag(sigma) V^T by the library's 3 x 3 SVD (factors
 *   proper or improper); d = +1 if det(U) det(V) > 0, else -1; R = U diag(1, 1, d) V^T; s = tr(R^T H) / sum |src_i - mu_s|^2 -- Umeyama's
 *   sigma_0 + sigma_1 +- sigma_2 evaluated as nine products, free of the sign and of the square root of the smallest singular value --
 *   or 1 when rigid; t = mu_d - s R mu_s.  One model per sample.  Degenerate samples give none:
 *   |(P2 - P1) x (P3 - P1)|^2 <= (1e-6)^2 x (longest squared side)^2 for the source triple or for the destination triple (relative,
 *   scale-free), and a scale that is not finite or not positive.
 *   Residual: inlier iff |s R src + t - dst|^2 <= thresh^2.
 *   Refit: the same closed form over the inliers of the best hypothesis (skipped below 3 inliers), adopted when it has at least as
 *   many inliers, and repeated on the adopted model's inliers while it strictly gains inliers (at most 4 fits).  Its sums take two
 *   passes (sum src, sum dst; then the 9 entries of H about the centroids and sum |src - mu_s|^2), each sum in a fixed order (256
 *   strided partials, partial k over the correspondences i = k mod 256 in ascending i, then a pairwise tree), which the GPU estimator
 *   reproduces.
 * Outputs: *s_out, R_out [9] row-major, t_out [3], inliers_out [M] and *n_inliers of the returned model; *n_inliers = -1 with s, R, t and
 * the mask zero when M < 3, no sample gave a model, or the best model has fewer than 3 inliers.
 * loftr_similarity_minimal exposes the minimal solver: src3 [3,3], dst3 [3,3] -> *n_solutions <= 1 model in *s, R [9], t [3] (zero
 * without one). */
int loftr_estimate_similarity(const double* src, const double* dst, long M, int with_scale, double thresh, float conf, unsigned seed,
                              double* s_out, double* R_out, double* t_out, uint8_t* inliers_out, long* n_inliers);
int loftr_similarity_minimal(const double* src3, const double* dst3, int with_scale, double* s, double* R, double* t, int* n_solutions);

/* loftr_estimate_similarity for every problem of a batch, on the GPU (csrc/similarity_gpu.hip).  CONTRACT: for every problem p the
 * result is the one loftr_estimate_similarity returns for that problem's correspondences with the same seed -- same n_inliers, same
 * inlier mask, s, R and t equal BIT FOR BIT (the outputs are fp64: there is no float rounding in between).
 *   src [M,3], dst [M,3] f64, m_bids [M] i64: device memory; the correspondences grouped by ascending problem id (problem p = the
 *   correspondences with m_bids == p, in order); with_scale, thresh, conf: as the host estimator; seed: one seed shared by every problem.
 * Outputs (device memory): s_out [P], R_out [P,9], t_out [P,3] f64; inliers_out [M] u8; n_inliers [P] i64, or -1 where the host
 * estimator returns -1 -- there s, R, t and the problem's mask are 0.
 * Stream-ordered on `stream`; the points never leave the device.  The call copies the per-hypothesis inlier counts to the host once,
 * replays the RANSAC loop there (the host estimator's own pow / log), copies one decision per problem back and waits for the stream
 * before it returns: two host round trips per batch, whatever P.  Workspace:
 * loftr_estimate_similarity_batched_workspace_bytes(M, P), about 125 kB per problem plus 49 bytes per correspondence.
 * Status: LOFTR_ERR_BAD_ARG for a null pointer, M < 0 or P < 0, P == 0 with M > 0, and for m_bids outside [0, P) or not grouped by
 * ascending problem (found on the device, reported at the call's own synchronisation; the outputs are then not written);
 * LOFTR_ERR_WORKSPACE for a short workspace; LOFTR_ERR_UNSUPPORTED for M >= 2^31 or P >= 2^31 / 1000.
 * M == 0 is valid (every problem gets -1); P == 0 and M == 0 is a no-op success. */
size_t loftr_estimate_similarity_batched_workspace_bytes(long M, int P);
int loftr_estimate_similarity_batched(const double* src, const double* dst, const long* m_bids, long M, int P, int with_scale, double thresh,
                                      float conf, unsigned seed, double* s_out, double* R_out, double* t_out, uint8_t* inliers_out,
                                      long* n_inliers, void* ws, size_t ws_bytes, void* stream);

/* Moving a model by one similarity (s, R, t), X' = s R X + t: loftr_transform_model_host (csrc/similarity.hip, host memory, synchronous)
 * and loftr_transform_model (csrc/similarity_gpu.hip, device memory, stream-ordered; a thread per point and a thread per image) run
 * one text, fp64 in a stated order without fused multiply-add, so the CPU chain and the GPU chain stay bit-equal.
 *   xyz [N,3] f32, T_cam_from_world [n_images,4,4] f64 row-major, posed [n_images] u8, s [1], R [9] row-major, t [3] f64 (pointers in
 *   the memory of the call's side).
 * Outputs: xyz_out [N,3] = f32(s (R_i0 X_0 + R_i1 X_1 + R_i2 X_2) + t_i), every row (a NaN row stays NaN); T_out [n_images,4,4]: for
 * a posed image R_c' = R_c R^T (rows left to right), t_c' = s t_c - R_c' t, bottom row 0 0 0 1, so that the camera coordinates of a
 * world point keep their direction and depths scale by s; an image that is not posed gets its input bits back, NaN included.
 * In place is allowed: xyz_out == xyz, T_out == T_cam_from_world.
 * Status: LOFTR_ERR_BAD_ARG for a null pointer (xyz / xyz_out only with N > 0, T / posed / T_out only with n_images > 0) or a negative
 * count; N == 0 and n_images == 0 is a no-op success. */
int loftr_transform_model_host(const float* xyz, long N, const double* T_cam_from_world, const uint8_t* posed, int n_images, const double* s,
                               const double* R, const double* t, float* xyz_out, double* T_out);
int loftr_transform_model(const float* xyz, long N, const double* T_cam_from_world, const uint8_t* posed, int n_images, const double* s,
                          const double* R, const double* t, float* xyz_out, double* T_out, void* stream);

/* ---- view overlap: image pairs by projected-point overlap (csrc/overlap_core.h holds every per-entry step) ------------------
 * Two images are worth matching when the points one of them observes project into the other within a viewing-angle and scale change
 * the matcher can bridge (the idea hloc ships as pairs_from_covisibility / pairs_from_poses).  overlap[i, j] counts the points that
 * source image i observes and that do so for target view j.  loftr_view_overlap_host (csrc/overlap.hip, host memory) DEFINES the result,
 * loftr_view_overlap (csrc/overlap_gpu.hip, device memory) reproduces it exactly: every output is an integer, a count is a sum of 0 / 1,
 * so no summation order needs fixing and identity rests on the per-entry predicate being one text.
 * Input: the visibility lists of the n source images -- vis_offsets [n+1] i64 over vis_point [V] i32 (point ids) --; the points xyz
 *   [T,3] f32 and point_ok [T] u8; the sources K_src [n,9], T_src [n,16] f64 (camera from world, row-major) and src_ok [n] u8; the m
 *   target views K_tgt [m,9], T_tgt [m,16] f64, tgt_ok [m] u8 and tgt_hw [m,2] f64 (H, W); border_px >= 0 (finite); cos_min in [-1, 1]
 *   (the cosine of the largest viewing-angle change, computed once by the caller and handed to both sides as the same double);
 *   max_scale2 >= 1 (the square of the largest ratio of apparent sizes; inf disables the test).  Arithmetic: fp64 without FMA
 *   contraction, + - * / and sqrt only; the camera table and the projection order are the triangulation's (tri::cam_table,
 *   tri::residual2: P = K [R | t], c = -R^T t, (a0 b0 + a1 b1) + a2 b2 as the dot product).
 *   1. A source i is valid iff src_ok[i] != 0 and its camera table is valid.  A target j likewise, and its H and W must be finite and
 *      positive.
 *   2. Entry p = vis_point[k] of a valid source is USABLE iff point_ok[p] != 0 and the three floats of xyz[p] are finite (exponent bits
 *      not all ones).  n_vis[i] is the number of usable entries; 0 for an invalid source.
 *   3. X = (double) xyz[p]; a = c_i - X, b = c_j - X, aa = a . a, bb = b . b, d = a . b.  A usable entry of source i COUNTS FOR the valid
 *      target j iff all of these hold, in this order (every comparison is written so that a NaN fails):
 *        z > 0, with x = (P0 . X) + P03, y = (P1 . X) + P13, z = (P2 . X) + P23 of target j;
 *        border <= u < W_j - border and border <= v < H_j - border, with u = x / z, v = y / z;
 *        d >= cos_min * sqrt(aa * bb);
 *        fxj^2 aa <= max_scale2 (fxi^2 bb) and fxi^2 bb <= max_scale2 (fxj^2 aa): the ratio of the apparent sizes f / distance, without a
 *        division; fx = K[0].
 *   4. overlap [n, m] i32: the number of entries of i that count for j.  An invalid source gives a zero row, an invalid target a zero
 *      column; i == j is not special.
 *   5. counts [8] i64: [0] the sum of n_vis, [1] error bits, [2] valid sources, [3] valid targets, [4] non-zero entries of overlap,
 *      the rest 0.
 *   6. Errors (counts[1]).  1: a vis_point outside [0, T); 2: vis_offsets that do not start at 0, end at V and ascend.
 * Status: LOFTR_ERR_BAD_ARG for null pointers (each only where its size is positive), negative sizes, border_px negative or not finite,
 *   cos_min outside [-1, 1], max_scale2 < 1, NaN parameters, entries without a list (n == 0 with V > 0); the host routine also for the two
 *   error bits, and it then writes the bits to counts[1], zero to the other counts and nothing else (the kernels raise counts[1] instead,
 *   read nothing through the bad value and leave overlap, n_vis and the other counts zero); LOFTR_ERR_UNSUPPORTED for V or T >= 2^31,
 *   n m > 2^31 entries, more than 65535 target tiles; LOFTR_ERR_WORKSPACE for a short workspace.
 * Out of scope: occlusion, visibility from the dense cells of the atlas, descriptor retrieval, a sparse output.  PARITY UNPINNED against
 *   hloc. */
int loftr_view_overlap_host(const long* vis_offsets, const int* vis_point, long V, const float* xyz, const uint8_t* point_ok, long T,
                            const double* K_src, const double* T_src, const uint8_t* src_ok, int n, const double* K_tgt,
                            const double* T_tgt, const uint8_t* tgt_ok, const double* tgt_hw, int m, double border_px, double cos_min,
                            double max_scale2, int* overlap, int* n_vis, long* counts);
/* The kernels: three memsets (overlap, n_vis, the counts) and three launches on the stream (0 the checks, 1 the view tables and n_vis
 * -- a wave per source, a thread per target --, 2 the counts -- a block per source and tile of LOFTR_OVERLAP_TILE targets: a lane owns
 * one target, the source's points are staged through LDS).  No host synchronisation unless stage_ms is given: NULL, or
 * LOFTR_OVERLAP_STAGES host floats that receive the GPU time of each launch (the call then waits for the stream).
 * Workspace: loftr_view_overlap_workspace_bytes(n, m): 224 bytes per source and per target; 0 for sizes out of range. */
#define LOFTR_OVERLAP_STAGES 3
#define LOFTR_OVERLAP_TILE 256
size_t loftr_view_overlap_workspace_bytes(int n, int m);
int loftr_view_overlap(const long* vis_offsets, const int* vis_point, long V, const float* xyz, const uint8_t* point_ok, long T,
                       const double* K_src, const double* T_src, const uint8_t* src_ok, int n, const double* K_tgt, const double* T_tgt,
                       const uint8_t* tgt_ok, const double* tgt_hw, int m, double border_px, double cos_min, double max_scale2, int* overlap,
                       int* n_vis, long* counts, void* ws, size_t ws_bytes, float* stage_ms, void* stream);

/* ---- input wire format (the step before the path; src/utils/dataset.py:78-89,111-118,149, megadepth.py:116-121) ----
 * From resized uint8 grayscale images to the tensors LoFTR.forward consumes: zero padding to [PH,PW] at the
 * bottom / right (pad_bottom_right), `float / 255`, the padding mask and its coarse version
 * (F.interpolate(mask, scale_factor=1/coarse_div, mode='nearest') = mask[d*y, d*x]).
 *   src [N, *, *] uint8 with byte pitches per image / per row; hw [N,2] int32 device: valid (h, w) <= (PH, PW);
 *   image [N,1,PH,PW] f32; mask [N,PH,PW] u8 or NULL; mask_c [N,PH/coarse_div,PW/coarse_div] u8 or NULL.
 * Decoding and cv2.resize stay with the caller (OpenCV; not reproducible without the library). */
/* ---- training-mode glue of the backbone (round 5; csrc/train_glue.hip) -------------------------------------------------------------
 * What sits between the convolutions of a TRAINING step of the ResNet-FPN (src/loftr/backbone/resnet_fpn.py:22-40,66-77,110-116) and was
 * PyTorch autograd until ABI 20.  fp32 tensors of logical shape [N, C, H, W] stored NCHW (channels_last = 0) or NHWC (channels_last = 1:
 * what the convolution nodes of the training path produce and consume -- no layout copy between a convolution and its BatchNorm; C % 4 == 0,
 * C <= 1024); HW = H * W; every reduction is a two-stage sum with float64 partials merged in a fixed order (deterministic).  Not used by the inference path (eval-mode BatchNorm is folded into the convolutions there).
 *
 * loftr_bn_train_fwd: nn.BatchNorm2d in .train() mode: mean / biased variance over (N, H, W) per channel, y = (x - mean) * invstd * gamma
 *   + beta (gamma / beta may be null: affine=False); mean [C], invstd [C] = 1 / sqrt(var + eps) are returned for the backward,
 *   var_unbiased [C] (may be null) is what the caller's running_var update takes (torch: momentum update with the UNBIASED variance).
 *   The reference trains with SyncBatchNorm (train.py:108): the same arithmetic over the union of the ranks' batches; one process here.
 * loftr_bn_train_bwd: dx, dgamma = sum dy * xhat, dbeta = sum dy (batch statistics: mean and variance depend on x).
 *   Workspace of both: loftr_bn_train_workspace_bytes(N, C, HW).
 * loftr_act_fwd: y = act(a + b) (b may be null; y may alias a): act 0 none, 1 ReLU, 2 LeakyReLU(slope) -- BasicBlock's relu(x + y)
 *   (resnet_fpn.py:40) and the heads' LeakyReLU (:70,:76).  loftr_act_bwd: dx = dy * act'(.) from the forward's OUTPUT y (the sign of the
 *   output is the sign of the input for a positive slope; dx is the gradient of a AND of b).
 * loftr_upsample2x_bilinear_fwd / _bwd: F.interpolate(x, scale_factor=2., mode='bilinear', align_corners=True) on N * C maps
 *   of H x W -> 2H x 2W (resnet_fpn.py:110,115) and its adjoint, evaluated as a gather (no atomics: deterministic, unlike torch's). */
size_t loftr_bn_train_workspace_bytes(int N, int C, long HW);
int loftr_bn_train_fwd(const float* x, int N, int C, long HW, int channels_last, const float* gamma, const float* beta, float eps, float* y,
                       float* mean, float* invstd, float* var_unbiased, void* ws, size_t ws_bytes, void* stream);
int loftr_bn_train_bwd(const float* dy, const float* x, int N, int C, long HW, int channels_last, const float* mean, const float* invstd,
                       const float* gamma, float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);
int loftr_act_fwd(const float* a, const float* b, long n, int act, float slope, float* y, void* stream);
int loftr_act_bwd(const float* dy, const float* y, long n, int act, float slope, float* dx, void* stream);
int loftr_upsample2x_bilinear_fwd(const float* x, int N, int C, int H, int W, int channels_last, float* y, void* stream);
int loftr_upsample2x_bilinear_bwd(const float* dy, int N, int C, int H, int W, int channels_last, float* dx, void* stream);

/* cv2.resize(image_u8, (dw, dh)) with the default INTER_LINEAR (dataset.py:108,146) on the device, one grayscale image.
 * PARITY UNPINNED: restates OpenCV 4.x's fixed-point bilinear (11-bit coefficients, half-pixel centres); OpenCV is not
 * in this image, so it is verified against the numpy restatement only (oracle/input_oracle.py). */
int loftr_resize_linear_u8(const uint8_t* src, int sh, int sw, long src_pitch, uint8_t* dst, int dh, int dw,
                           long dst_pitch, void* stream);
int loftr_pack_gray_u8(const uint8_t* src, long src_image_pitch, long src_row_pitch, const int* hw, int N, int PH,
                       int PW, float* image, uint8_t* mask, uint8_t* mask_c, int coarse_div, void* stream);

/* ---- multi-GPU: the one data-path collective (SURVEY.md §8(b),(e)) -----------------------------------
 * Replaces the reference's result merge across DDP ranks (test.py:65 + src/lightning/data.py:315 shard the pairs,
 * src/utils/comm.py:113-219 gathers pickled results over gloo): pairs are independent, so all a rank needs from
 * the others is how many matches each of THEIR pairs produced -- an RCCL all-gather of int32[n] per rank over xGMI
 * on the caller's stream (latency bound; no host round trip).  counts_out[r*n + k] = counts_in[k] of rank r.
 * The communicator is an opaque handle bound to the HIP device current at creation; the 128-byte unique id comes
 * from loftr_rccl_unique_id on one rank and reaches the others through the caller's control plane.
 * librccl is dlopen'ed on first use: LOFTR_ERR_COMM if it is missing or any RCCL call fails. */
#define LOFTR_RCCL_ID_BYTES 128
int loftr_rccl_unique_id(char* id_out, size_t id_bytes);
int loftr_rccl_comm_create(const char* id, size_t id_bytes, int rank, int world, void** comm_out);
int loftr_rccl_comm_info(void* comm, int* rank_out, int* world_out);
int loftr_rccl_comm_destroy(void* comm);
int loftr_rccl_allgather_counts(void* comm, const int32_t* counts_in, int32_t* counts_out, int n, void* stream);

/* ---- debug / A-B switches (process-global; the library reads NO environment variable) -------------
 * Named integer switches that select an alternative schedule of the same arithmetic for A/B measurements and tests:
 *   "encoder_schedule"  1: loftr_transformer_fwd runs the coarse level as scheduled launches; 0: call by call in the reference's order
 *   "conv_persist_cap"  0: persistent convolution grids span the device's CUs; n >= 8: at most n workgroups (tests: many tiles each)
 *   "wgrad_chunk"       0: split-K chunk of the weight-gradient GEMMs chosen by shape; n > 0: forced
 *   "reduce_tall"       1: tall partial-sum reductions use the tall kernel; 0: the generic one
 *   "conv_duo"          1: 3x3 / stride-1 convolutions of 128 k / 192 / 224 output columns run conv3x3_duo_kernel; 0: the generic conv3x3_kernel
 *   "conv_rem"          1: loftr_conv_bn_act_prepared_scratch takes the remainder form where it applies; 0: never
 *   "conv_patch"        1: 3x3 / stride-1 convolutions run the patch kernels; 0: the implicit-GEMM kernel of the strided / 1x1 layers
 *   "pct_grid"          0: the persistent coarse transformer runs 256 workgroups (one per CU); n > 0: n workgroups
 *   "pct_quota"         0: its workgroups stay until the queue is empty; n > 0: a workgroup leaves after n work items (yielding variant)
 *   "pct_skip"          0; bit t: work items of type t (0 X, 1 K, 2 F) are popped and signalled but NOT executed (queue tests: wrong results)
 *   "fine_waves"        0: fine_pair_kernel runs four or eight waves per workgroup by the match count; 4 / 8: forced (same bits either way)
 * Unknown key: LOFTR_ERR_BAD_ARG.  Results never depend on a switch beyond the last bits of a floating-point sum order. */
int loftr_hip_debug_set(const char* key, int value);
int loftr_hip_debug_get(const char* key, int* value, int* default_value);

/* ---- per-kernel timing (profiling aid; process-global like the debug switches) ---------------
 * When bit `id` of the mask is set, every launch of that kernel is bracketed by hipEvents
 * recorded on the launch stream (up to 4096 launches between reads).  Replaces the reference's
 * InferenceProfiler (src/utils/profiler.py:7-28: cuda.synchronize()-bracketed wall clocks).
 * loftr_hip_timing_read synchronises the recorded events and returns the accumulated GPU time
 * (ms) and launch count of kernel `id`; reset != 0 clears the accumulators. */
int loftr_hip_timing_enable(unsigned mask);
int loftr_hip_timing_kernel_count(void);
const char* loftr_hip_timing_kernel_name(int id);
int loftr_hip_timing_read(int id, double* total_ms, long long* launches, int reset);

/* ---- fp16-range guard (debug aid, process-global like the timing switch) -----------------------
 * The GEMM chain holds every operand as two fp16 numbers (csrc/gemm.h).  Weights, convolution filters and tensors entering through
 * loftr_linear_fwd / loftr_sp_from_f32_scaled are pre-scaled by powers of two and cannot overflow; the fine-level transformer
 * rescales its windows at run time (csrc/fine_fused.hip).  Activations that enter the chain UNSCALED -- the coarse feature maps after
 * the positional encoding, the coarse descriptors at the matcher, the fine preprocess inputs -- must stay below the fp16 maximum
 * 65504: beyond it the affected products are inf / NaN where the fp32 reference (src/loftr/loftr.py:56-75) is still finite.  With the
 * guard on, every such conversion is followed by a (synchronous) scan and the entry point returns LOFTR_ERR_RANGE instead. */
int loftr_hip_range_check_enable(int on);

/* ---- building block exposed for tests / profiling ------------------------------------------
 * out[M,N] = A[M,K] @ Wt[N,K]^T  (the fp32-accurate split-fp16 MFMA GEMM every linear layer above
 * is built on). */
size_t loftr_linear_workspace_bytes(int M, int N, int K);
int loftr_linear_fwd(const float* a, const float* w, float* out, int M, int N, int K,
                     void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LOFTR_HIP_H_ */
