/* libopp_hip.so -- C ABI of the MI355X (gfx950) implementation of the OnePose++ 2D-3D
 * matching forward.
 *
 * This is the drop-in boundary UNDER the Python module `onepose_plus_plus_amd.OnePosePlus_model`
 * (which mirrors the reference's `OnePosePlus_model(config)(data)` API,
 * /root/reference/src/models/OnePosePlus/OnePosePlusModel.py:25-201).  The reference is pure
 * Python on PyTorch, so there is no upstream FFI to bind; every entry point below cites the
 * reference code whose GPU work it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - all tensor pointers are DEVICE pointers to fp32 unless noted; int64 = `long long`.
 *  - the library never allocates device memory: the caller passes a workspace and the packed
 *    weight blob (sizes from the *_bytes queries) and owns every buffer.
 *  - every call enqueues work on `stream` (a hipStream_t passed as void*) and returns
 *    without synchronising; 0 = ok, negative = error (message via opp_last_error()).
 *  - a workspace is never read before the call has written it, nothing is written outside workspace[0, *_workspace_bytes) and
 *    the documented extent of each output, and a workspace that is too small is refused with -4 before anything is launched.
 *  - activations are NHWC ("pixel-major, channel contiguous"); the 196-channel stages are
 *    padded to 224 channels with zeros.
 *  - batch size is 1 (the reference's inference path, inference_OnePosePlus_worker.py:52-60).
 */
#ifndef OPP_HIP_H
#define OPP_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OPP_MAX_LAYERS 16

/* The `model.OnePosePlus` block of configs/experiment/inference_onepose.yaml:26-109, reduced to
 * the values the kernels depend on. */
typedef struct opp_config {
  int initial_dim;         /* loftr_backbone.resnetfpn.initial_dim (128) */
  int block_dims[3];       /* loftr_backbone.resnetfpn.block_dims (128,196,256) */
  int kpt_enc_enable;      /* keypoints_encoding.enable */
  int kpt_enc_dims[3];     /* keypoints_encoding.keypoints_encoder (32,64,128) */
  int pos_enc_enable;      /* positional_encoding.enable */
  int coarse_d_model;      /* loftr_coarse.d_model (256) */
  int coarse_nhead;        /* loftr_coarse.nhead (8) */
  int coarse_n_layers;     /* len(layer_names) * layer_iter_n (6) */
  int coarse_is_cross[OPP_MAX_LAYERS]; /* 0 = self, 1 = cross */
  int fine_d_model;        /* loftr_fine.d_model (128) */
  int fine_nhead;          /* loftr_fine.nhead (8) */
  int fine_n_layers;       /* (2) */
  int fine_is_cross[OPP_MAX_LAYERS];
  int fine_window;         /* loftr_fine.window_size (5) */
  float match_thr;         /* coarse_matching.thr */
  int match_border_rm;     /* coarse_matching.border_rm */
  float match_temperature; /* coarse_matching.dual_softmax.temperature */
  /* Not a reference key: arithmetic of the conv / Linear / score GEMMs (fp32 in, fp32 accumulate, fp32 out in
   * every mode).
   * 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32, bit-for-bit an fmaf chain).
   * 3 = bf16x3 split (the module default): every operand x is carried EXACTLY as hi + mid + lo bf16
   *     (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid): 24 significant bits, fp32 exponent range, no
   *     range restriction), six bf16 MFMAs per product (the dropped mid*lo, lo*mid, lo*lo terms are <= 2^-26 |a||b|,
   *     below fp32's own rounding), 6/16 of the fp32 MFMA cycles.  Not narrower than fp32.
   * 1 = fp16x2 split (NARROWER than fp32; TUNING LIBRARY ONLY since round 6 -- the product build has no fp16x2 kernels and
   *     opp_create refuses 1 and 2, see opp_supports_precision): x ~ hi + lo fp16 (22-bit mantissa), three fp16 MFMAs
   *     per product, 3/16 of the fp32 MFMA cycles.  Activations must stay inside the fp16 range (|x| < 65504;
   *     the kernels flag non-finite outputs, see opp_forward_coarse `count[1]`), values below 2^-3 keep an
   *     absolute 2^-25 error; weights are pre-scaled per matrix and unrestricted.  The coarse score GEMM stays fp32.
   * 2 = as 1, and the score GEMM runs on the fp16x2 path too (image tokens split once per image). */
  int gemm_precision;
  /* Not a reference key: what the automatic GEMM / conv tile choice minimises.  0 = the duration of each launch
   * (one forward at a time: lowest latency); 1 = the CU time each launch occupies (several forwards in flight on
   * separate streams -- MatcherPool, bench.py --streams > 1 -- where other forwards' kernels fill idle CUs: +3.5...6.5 %
   * images/s with three forwards in flight, -9 % for a forward running alone).  Results are bit-identical. */
  int tile_policy;
  /* Not a reference key: with gemm_precision 3 every LoFTREncoderLayer behind its Q/K/V projection (attention apply, merge,
   * norm1, mlp.0, ReLU, mlp.2, norm2, residual; transformer.py:80-94) runs as ONE kernel whose activations stay in LDS:
   * 2 (the module default) = 64-token tiles at the coarse level (one round of workgroups at 9096 tokens; csrc/enc_layer64.hip),
   * 32-token tiles at the fine level; 1 = 32-token tiles everywhere (csrc/enc_chain.hip); 0 = one launch per Linear.
   * Bit-identical results in all three. */
  int encoder_fusion;
  /* Not a reference key: coarse-matcher variant under gemm_precision 3 (both operands of the score GEMM pre-split once and
   * staged global -> LDS by LDS-DMA, 4-wave workgroups on 128 x 128 tiles, two workgroups per CU; csrc/gemm_ss.hip).
   * 2 (the module default) = ONE sweep: dual-softmax statistics + score matrix, confidences then formed in place;
   * 1 = TWO sweeps (statistics only, then the tiles recomputed and the confidences written once: one N x L write instead of
   *     write + read + write, at twice the MFMA work); 0 = the r02 path (opp_gemm_kernel, image tokens as pre-split weights). */
  int score_two_sweep;
  /* Not a reference key: 1 (the module default) = opp_forward_coarse runs the FPN fine branch of the backbone (layer2 / layer1
   * lateral + output convolutions -> feat_f, needed by the fine stage only) on a side HIP stream next to the coarse level
   * (tokens, transformer, matcher), forking after layer3_outconv and joining before it returns: the short, CU-starved launches
   * of the coarse level and the chip-filling convolutions of the fine branch share the device.  Results are identical (same
   * kernels, same order within each branch); the workspace holds both branches' buffers at once.  0 = one stream. */
  int fpn_overlap;
  /* loftr_coarse.attention / loftr_fine.attention (transformer.py:32-40): 0 = "linear" (LinearAttention, elu + 1 feature map; the default,
   * what a zero-initialised config selects), 1 = any other value upstream = FullAttention, softmax(Q K^T / sqrt(D)) V
   * (linear_attention.py:64-95; csrc/full_attention.hip).  With full attention at a level every layer there runs the plain Q/K/V projection,
   * opp_full_attention's kernels and the unchanged merge / norm / MLP tail; the per-object prefix is off when the coarse level is full
   * (opp_object_prefix_bytes = 0) and a query mask is refused (upstream cannot run a masked forward with a cross layer either).
   * opp_create refuses other values (OPP_ERR_UNSUPPORTED). */
  int coarse_attention;
  int fine_attention;
  /* loftr_coarse.norm_method / loftr_fine.norm_method (transformer.py:49-54): 0 = "layernorm" (the default), 1 = "instancenorm" =
   * nn.InstanceNorm1d(d_model) applied to [N, L, C] tokens = the per-token normalisation over the C channels without affine: the level's
   * norm1 / norm2 names are not in the weight table, the packed affine slots hold ones and zeros and every layer kernel runs unchanged. */
  int coarse_norm;
  int fine_norm;
  /* loftr_coarse.rezero / loftr_fine.rezero is a number (transformer.py:61-63, :94: x + res_weight * message): 1 = every layer of the level
   * has a `res_weight` [1] entry in the weight table (in front of q_proj.weight, as in the reference state dict); opp_pack_weights folds it
   * into the packed norm2 affine (gamma2 * w, beta2 * w), so the residual add of the layer kernels needs no further operand. */
  int coarse_rezero;
  int fine_rezero;
  /* keypoints_encoding.norm_method (position_encoding.py:69-74): 0 = "instancenorm" (per-point normalisation over the channels, no affine;
   * the default), 1 = "layernorm" (the same normalisation + nn.LayerNorm's affine: encoder.{1,4,7}.{weight,bias} join the weight table). */
  int kpt_norm;
  /* coarse_matching.feat_norm_method (coarse_matching.py:46-54): 0 = "sqrt_feat_dim" (scores divided by C; the default), 1 = "none" / None
   * (scores as they are). */
  int feat_norm;
  /* Not a reference key of the 2D-3D model: the layer schedule of the 2D-2D matcher (LoFTR, onepose_plus_plus_amd/loftr.py).  0 (what
   * every 2D-3D configuration has) = a cross layer updates both streams from each other's PRE-update tokens (quirk q6); 1 = sequential:
   * a cross layer updates stream 0 from stream 1, then stream 1 from the UPDATED stream 0, at both levels.  Each stream's q, k, v are
   * still projected once per layer (q of stream 0 and q | k | v of stream 1 first, k | v of stream 0 after its update).  Runs with
   * encoder_fusion 0 and linear attention only (opp_create refuses anything else), in both arithmetics, and admits fine windows up to
   * 9 x 9 (81 + 81 tokens per match through opp_fine2d).  Honoured by opp_transformer and opp_fine2d, the stages of the 2D-2D matcher; the
   * 2D-3D entries opp_forward_coarse, opp_fine and opp_fine_patches refuse such a context.  With more than one segment the schedule runs
   * d_model 128 / 8 heads and at most 81 tokens per stream only (one workgroup per segment); other shapes are refused. */
  int cross_sequential;
} opp_config;

typedef struct opp_ctx opp_ctx;

const char* opp_last_error(void);
int opp_version(void);
/* sha256 (hex) of the sources this binary was built from (every file of csrc/ + this header), baked in by the build;
 * the Python binding compares it with the sources next to the library and refuses a stale binary. */
const char* opp_source_hash(void);
/* 1 when this binary can run opp_config.gemm_precision `p` (0 fp32 and 3 bf16x3: always; 1 / 2 fp16x2: only a library built with
 * `python -m onepose_plus_plus_amd.build --tuning`), else 0.  Not a reference interface: the reference has one arithmetic (fp32). */
int opp_supports_precision(int gemm_precision);

/* ---- model handle + weights -------------------------------------------------------------
 * Replaces: OnePosePlus_model.__init__ + load_state_dict (OnePosePlusModel.py:26-94,
 * src/inference/inference_OnePosePlus.py:28-38).  Weight tensors are given in the reference
 * state-dict order without the BatchNorm `num_batches_tracked` counters; opp_weight_name(i)
 * returns the state-dict key expected at index i. */
int opp_create(const opp_config* cfg, opp_ctx** out);
void opp_destroy(opp_ctx* ctx);
/* query_image_mask of the CURRENT sample (OnePosePlusModel.py:158: data['query_image_mask'].flatten(-2)): device
 * array of L = hc*wc floats, 1 = valid image cell, 0 = padding; NULL (default) = no mask.  Applies to the coarse
 * transformer (phi(Q), phi(K), V rows of masked image tokens are zeroed, linear_attention.py:49-53) and to the coarse
 * matcher (-1e9 added to the masked columns of the score matrix, coarse_matching.py:108-114) in every later call made
 * through this ctx: opp_transformer (which = 0, n_seg = 1), opp_coarse_match, opp_forward_coarse. */
int opp_set_query_mask(opp_ctx* ctx, const float* mask);
/* B > 1 (quirk of normalize_3d_keypoints, utils/normalize.py:20-21): the 3D keypoints of EVERY batch element are scaled
 * by the bounding-box extent of batch element 0 and centred on their own mean.  kpts0 [n0][3] = the keypoints of
 * batch element 0 (NULL = each cloud uses its own extent, the B = 1 behaviour).  Applies to opp_encode_points,
 * opp_coarse_tokens and opp_forward_coarse. */
int opp_set_keypoint_extent_ref(opp_ctx* ctx, const float* kpts0, int n0);
/* bf16x3 arithmetic, opt-in (default off; OPP_CONV_TAIL=1 turns it on for every context): the convolutions with 196 output channels
 * (backbone/resnet.py:88-124, block_dims[1]) as a 192-column body on the MFMA kernel (tile 128 x 192, no padded column sub-tile) + their
 * last 4 columns as fp32 FMA chains on the vector ALU (csrc/conv_tail.hip).  Same parity bar; measured slower with one forward in flight
 * and equal with three, hence not the default. */
int opp_set_conv_tail(opp_ctx* ctx, int on);
/* fp16x2 range guard (gemm_precision 1 / 2 only; a no-op otherwise): `flag` is a device int that every stage
 * enqueued through this ctx ORs with 1 when an fp16x2 GEMM produced a non-finite value, i.e. an activation left the
 * fp16 range (|x| >~ 1.3e5) -- or the input itself was not finite.  The caller zeroes it, reads it after the
 * stream work completed, and re-runs in another arithmetic (the Python module switches to bf16x3).  NULL disables. */
int opp_set_status_flag(opp_ctx* ctx, int* flag);
int opp_num_weights(const opp_ctx* ctx);
const char* opp_weight_name(const opp_ctx* ctx, int i);
long long opp_weight_numel(const opp_ctx* ctx, int i);
size_t opp_packed_weights_bytes(const opp_ctx* ctx);
/* folds eval-mode BatchNorm into the convolutions, re-lays conv weights tap-major/NHWC with
 * channel padding, concatenates q/k/v projections, transposes the keypoint MLP. */
int opp_pack_weights(opp_ctx* ctx, const float* const* weights, int n_weights, void* packed,
                     size_t packed_bytes, void* stream);
/* What the NEXT opp_pack_weights lays out: 0 (default) = everything; 1 = a training step: only the backbone convolutions WITHOUT a
 * BatchNorm behind them (the others are packed raw by opp_pack_train_weights; the training graph's transformer / keypoint-encoder
 * nodes, onepose_plus_plus_amd/train_autograd.py, read the parameters directly) -- the per-step repacking is then ~80 launches
 * shorter.  opp_backbone / opp_transformer / opp_coarse_tokens / opp_encode_points / opp_forward_coarse / opp_fine refuse to run
 * until the weights are packed with scope 0 again. */
int opp_set_pack_scope(opp_ctx* ctx, int scope);

/* ---- training-mode forward of the backbone ------------------------------
 * PL_OnePosePlus.training_step runs the same module in train() mode (src/lightning_model/
 * OnePosePlus_lightning_model.py:54-81): every nn.BatchNorm2d of the ResNet-FPN then normalises with the statistics of
 * the current batch over (B, H, W) and updates its running statistics (backbone/resnet.py:25-26, :101-113; plain
 * BatchNorm, no SyncBN upstream).  opp_pack_train_weights packs the backbone convolutions WITHOUT the folded
 * BatchNorm (after opp_pack_weights, same `weights` table; the BatchNorm affine tensors of that table are read in
 * place during the forward and must stay alive).  opp_backbone_train: image [B][H][W]; feat_c [B][H/8][W/8][256],
 * feat_f [B][H/2][W/2][128] (NHWC); bn_stats (may be NULL) receives, for BatchNorm layer i of opp_bn_layer_name(i),
 * 512 floats: [0, C) the batch mean, [C, 2C) the UNBIASED batch variance -- what the caller folds into
 * running_mean / running_var with momentum 0.1 like the BatchNorm2d default.  Forward only (no backward here). */
int opp_num_bn_layers(const opp_ctx* ctx);
const char* opp_bn_layer_name(const opp_ctx* ctx, int i);      /* state-dict prefix, e.g. "backbone.layer1.0.bn1" */
int opp_bn_layer_channels(const opp_ctx* ctx, int i);
size_t opp_packed_train_weights_bytes(const opp_ctx* ctx);
int opp_pack_train_weights(opp_ctx* ctx, const float* const* weights, int n_weights, void* packed,
                           size_t packed_bytes, void* stream);
size_t opp_backbone_train_workspace_bytes(const opp_ctx* ctx, int B, int H, int W);
int opp_backbone_train(opp_ctx* ctx, const float* image, int B, int H, int W, float* feat_c, float* feat_f,
                       float* bn_stats, void* workspace, size_t workspace_bytes, void* stream);

/* ---- stages ---------------------------------------------------------------------------- */
size_t opp_backbone_workspace_bytes(const opp_ctx* ctx, int H, int W);
/* ResNetFPN_8_2.forward (backbone/resnet.py:141-164).  image [H][W] in [0,1];
 * feat_c NHWC [H/8][W/8][256] (x3_out), feat_f NHWC [H/2][W/2][128] (x1_out). */
int opp_backbone(opp_ctx* ctx, const float* image, int H, int W, float* feat_c, float* feat_f,
                 void* workspace, size_t workspace_bytes, void* stream);

/* OnePosePlusModel.py:137-156: tokens[0:L] = feat_c + pe (pe NHWC [L][C], may be NULL),
 * tokens[L:L+N] = bank_c[C][N]^T + MLP(normalize_3d_keypoints(kpts)).  tokens [L+N][C]. */
int opp_coarse_tokens(opp_ctx* ctx, const float* feat_c, const float* pe, int L, const float* kpts,
                      const float* bank_c, int n_points, float* tokens, void* workspace,
                      size_t workspace_bytes, void* stream);

/* The 3D-point half of the tokens above on its own: it depends only on the object (keypoints +
 * coarse bank), not on the query image, so a caller that keeps the bank resident encodes it once
 * per object and passes the result to opp_forward_coarse.  tokens3d [N][C]. */
int opp_encode_points(opp_ctx* ctx, const float* kpts, const float* bank_c, int n_points,
                      float* tokens3d, void* workspace, size_t workspace_bytes, void* stream);

/* Image-independent prefix of the coarse transformer of a RESIDENT object (round 5).  With layer_names = ["self", "cross", ...]
 * (loftr_module/transformer.py:147-160) layer 0 updates the 3D-point stream from itself only, and in layer 1 both streams read the
 * PRE-update tokens of the other one, so the 3D stream after layer 0, its layer-1 q / k / v projections and its layer-1 KV / Ksum
 * depend on (keypoints3d, coarse bank) alone -- OnePosePlusModel.py:160-164 recomputes them per image.  opp_object_prefix evaluates
 * them once from the tokens of opp_encode_points into a caller-owned blob of opp_object_prefix_bytes() bytes (16-byte aligned;
 * 0 = this configuration -- another arithmetic, encoder_fusion != 2, other layer names -- has no prefix and every layer is evaluated
 * per image); opp_set_object_prefix hands the blob to the NEXT opp_forward_coarse calls of this ctx (used when tokens3d_pre is
 * given and n_points matches; NULL = off).  Results are bit-identical with and without it (rows are independent in every kernel
 * of a layer, the KV reduction is chunked per stream). */
size_t opp_object_prefix_bytes(const opp_ctx* ctx, int n_points);
size_t opp_object_prefix_workspace_bytes(const opp_ctx* ctx, int n_points);
int opp_object_prefix(opp_ctx* ctx, const float* tokens3d, int n_points, void* prefix, size_t prefix_bytes, void* workspace,
                      size_t workspace_bytes, void* stream);
int opp_set_object_prefix(opp_ctx* ctx, const void* prefix, int n_points);

/* LocalFeatureTransformer.forward (loftr_module/transformer.py:133-171), in place on
 * tokens = [n_seg*len0 rows of stream "2D" ; n_seg*len1 rows of stream "3D"] x d_model.
 * which = 0: loftr_coarse, 1: loftr_fine. */
size_t opp_transformer_workspace_bytes(const opp_ctx* ctx, int which, int n_seg, int len0, int len1);
int opp_transformer(opp_ctx* ctx, int which, float* tokens, int n_seg, int len0, int len1,
                    void* workspace, size_t workspace_bytes, void* stream);
/* Test aid: byte offsets, inside the workspace of opp_transformer for the same arguments, of the linear attention's reduced
 * KV [2][n_seg][d_model * d_head] and Ksum [2][n_seg][d_model] (stream 0 first).  After opp_transformer they hold the sums the LAST
 * layer applied (linear attention only). */
int opp_transformer_kv_offsets(const opp_ctx* ctx, int which, int n_seg, int len0, int len1, size_t* kv_offset, size_t* ks_offset);

/* CoarseMatching.forward + get_coarse_match, inference branch (utils/coarse_matching.py:76-242).
 * feat2d [L][C], feat3d [N][C]; conf [N][L] is written (data['conf_matrix']).  Outputs have
 * capacity N; *count (device int) receives M.  base_scale = H/hc; query_scale = device pointer to
 * data['query_image_scale'][0] = (h_scale, w_scale) or NULL. */
size_t opp_coarse_match_workspace_bytes(const opp_ctx* ctx, int n_points, int L);
int opp_coarse_match(opp_ctx* ctx, const float* feat3d, const float* feat2d, int n_points, int hc,
                     int wc, const float* kpts, float base_scale, const float* query_scale, float* conf,
                     long long* i_ids, long long* j_ids, float* mconf, float* mkpts_c,
                     float* mkpts_3d, int* count, void* workspace, size_t workspace_bytes,
                     void* stream);

/* Whole coarse level in one call: backbone -> tokens -> loftr_coarse -> coarse matching
 * (OnePosePlusModel.py:116-167).  feat_f is kept for the fine stage; feat_f = NULL says the caller runs no fine
 * stage (fine_matching.enable = False, OnePosePlusModel.py:169-176): the fine map is then dead -- not an output, read by
 * nothing -- and the FPN branch that produces it is not launched (every output of this call is unchanged).
 * tokens3d_pre: optional result of opp_encode_points for this object (NULL = encode kpts/bank_c here). */
size_t opp_forward_coarse_workspace_bytes(const opp_ctx* ctx, int H, int W, int n_points);
int opp_forward_coarse(opp_ctx* ctx, const float* image, int H, int W, const float* pe,
                       const float* kpts, const float* bank_c, const float* tokens3d_pre, int n_points,
                       float base_scale, const float* query_scale, float* feat_f, float* conf, long long* i_ids,
                       long long* j_ids, float* mconf, float* mkpts_c, float* mkpts_3d, int* count,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Fine level (OnePosePlusModel.py:179-201): FinePreprocess window gather, loftr_fine,
 * FineMatching.  feat_f NHWC [Hf][Wf][d_fine]; bank_f [d_fine][N] (RAW fine bank, quirk q8);
 * ids are the first M entries of the coarse outputs.  base_scale = H/Hf; query_scale as above.
 * run_transformer = config loftr_fine.enable.  The workspace must hold opp_fine_workspace_bytes whether run_transformer is set or not. */
size_t opp_fine_workspace_bytes(const opp_ctx* ctx, int n_matches);
int opp_fine(opp_ctx* ctx, const float* feat_f, int Hf, int Wf, const float* bank_f, int n_points,
             const long long* i_ids, const long long* j_ids, int n_matches, int hc, int wc,
             const float* mkpts_c, float base_scale, const float* query_scale, int run_transformer,
             float* expec_f, float* mkpts_f, void* workspace, size_t workspace_bytes, void* stream);

/* Match-driven fine branch (round 5; eval mode, where the folded BatchNorm makes every backbone operator pointwise in its inputs).
 * The 1/2-resolution half of the FPN fine branch -- layer1_outconv + the bilinear residual, layer1_outconv2 (backbone/resnet.py:154-157):
 * 78 of the 337 GFLOP of a 512 x 512 forward -- is consumed only through the W x W windows around the M coarse matches
 * (loftr_module/fine_preprocess.py:41-55).  opp_set_fine_patch_buffers(x1, x2_out) makes the NEXT opp_forward_coarse calls with
 * feat_f = NULL keep x1 [H/2][W/2][pad32(block_dims[0])] and x2_out [H/4][W/4][pad32(block_dims[1])] (NHWC; element counts from
 * opp_fine_patch_buffer_floats(ctx, H, W, 0 / 1)) in the caller's buffers and stop the backbone there (NULL, NULL = off).  Once the
 * match count is known the caller either
 *   - runs opp_fine_patches: the three convolutions as VALID convolutions over a (W+4)^2 -> (W+2)^2 -> W^2 patch pyramid per match
 *     (49 MFLOP per match) on the same kernel, weights and K order as the dense maps, written straight into the window tokens of
 *     loftr_fine, then the fine transformer and FineMatching exactly as opp_fine; or
 *   - for many matches (break-even ~ 1000 at 512 x 512) completes the dense map with opp_backbone_fine_branch and calls opp_fine.
 * Both give the bits of the one-call path (tests/test_e2e_gpu.py::test_match_driven_fine_branch_*). */
int opp_set_fine_patch_buffers(opp_ctx* ctx, float* x1, float* x2_out);
size_t opp_fine_patch_buffer_floats(const opp_ctx* ctx, int H, int W, int which);
size_t opp_fine_patches_workspace_bytes(const opp_ctx* ctx, int n_matches);
int opp_fine_patches(opp_ctx* ctx, const float* x1, const float* x2_out, int H, int W, const float* bank_f, int n_points,
                     const long long* i_ids, const long long* j_ids, int n_matches, int hc, int wc, const float* mkpts_c,
                     float base_scale, const float* query_scale, int run_transformer, float* expec_f, float* mkpts_f,
                     void* workspace, size_t workspace_bytes, void* stream);
size_t opp_backbone_fine_branch_workspace_bytes(const opp_ctx* ctx, int H, int W);
int opp_backbone_fine_branch(opp_ctx* ctx, const float* x1, const float* x2_out, int H, int W, float* feat_f, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- 2D-2D matching (LoFTR as the reference's LoFTR_for_OnePose_Plus strings it together, src/KeypointFreeSfM/loftr_for_sfm/loftr.py:16-128;
 * the LoFTR submodule itself is absent from the reference: these entries follow the published LoFTR, parity unpinned) -------------------
 * opp_image_tokens: tokens [L][coarse_d_model] = feat_c + pe (pe may be NULL: a copy), the coarse tokens of one image.
 * opp_match2d: CoarseMatching of two images.  f0 [L0][C], f1 [L1][C] (L0 = h0c * w0c, L1 = h1c * w1c): sim = <f0 / sqrt(C), f1 / sqrt(C)> /
 * match_temperature (exactly as configured), conf [L0][L1] = softmax(sim, rows) * softmax(sim, columns) is written; a pair (i, j) is kept
 * when conf > match_thr, conf is the maximum of its row and of its column, and neither cell lies within match_border_rm cells of ANY of the
 * four edges of its own grid; a row with several such j keeps the first; output in ascending i with capacity L0, *count (device int) = M.
 * mkpts0_c [M][2] = (i % w0c, i / w0c) * base_scale * scale0[[1, 0]], mkpts1_c likewise from j, w1c, scale1 (scale* = device pointers to
 * (h_scale, w_scale), or NULL = 1).  The score GEMM runs in the context's arithmetic (image 1's tokens pre-split under bf16x3).
 * opp_fine2d: window gather of BOTH 1/2-resolution maps (NHWC [Hf][Wf][fine_d_model], W x W cells at `stride` = Hf / hc around coarse
 * cells i_ids[m] / j_ids[m], zeros outside the map), loftr_fine on M segments of W^2 + W^2 tokens, then the expectation head of opp_fine
 * with the CENTRE token of window 0 in the place of the 3D point token: expec_f [M][3], mkpts1_f = mkpts1_c + expec_f[:, :2] * (W / 2) *
 * base_scale * scale1[[1, 0]].  Wf = w*c * stride and Hf a multiple of stride are required.  M <= 0 returns at once.  Both workspace-taking entries follow the workspace contract above. */
int opp_image_tokens(opp_ctx* ctx, const float* feat_c, const float* pe, int L, float* tokens, void* stream);
size_t opp_match2d_workspace_bytes(const opp_ctx* ctx, int L0, int L1);
int opp_match2d(opp_ctx* ctx, const float* f0, const float* f1, int h0c, int w0c, int h1c, int w1c, float base_scale,
                const float* scale0, const float* scale1, float* conf, long long* i_ids, long long* j_ids, float* mconf,
                float* mkpts0_c, float* mkpts1_c, int* count, void* workspace, size_t workspace_bytes, void* stream);
size_t opp_fine2d_workspace_bytes(const opp_ctx* ctx, int n_matches);
int opp_fine2d(opp_ctx* ctx, const float* feat_f0, int Hf0, int Wf0, const float* feat_f1, int Hf1, int Wf1, const long long* i_ids,
               const long long* j_ids, int n_matches, int w0c, int w1c, int stride, const float* mkpts1_c, float base_scale,
               const float* scale1, float* expec_f, float* mkpts1_f, void* workspace, size_t workspace_bytes, void* stream);

/* ---- training step: coarse focal loss (Loss.compute_coarse_loss, src/lightning_model/losses.py:18-55) -------------
 * conf [n] fp32 (the B x N x L confidence matrix, 16-byte aligned), conf_gt [n] int16 (0 / 1; other values are ignored
 * like the reference's `== 1` / `== 0` masks), weight [n] or NULL.
 * forward: sums[4] (device, fp64) = { sum of the positive terms, sum of the negative terms, #positives, #negatives };
 *   term_pos = -alpha (1 - c)^gamma log c, term_neg = -(1 - alpha) c^gamma log(1 - c), c = clamp(conf, 1e-6, 1 - 1e-6);
 *   the caller forms pos_weight * mean_pos + neg_weight * mean_neg (losses.py:44-53) from them without a host sync.
 * backward: grad_conf [n] = d loss / d conf given scales[2] (device) = { g * pos_weight / #pos, g * neg_weight / #neg },
 *   g the incoming gradient of the scalar loss; zero where the clamp saturates. */
size_t opp_focal_loss_workspace_bytes(size_t n);
int opp_focal_loss_forward(const float* conf, const short* conf_gt, const float* weight, size_t n, float alpha,
                           float gamma, double* sums, void* workspace, size_t workspace_bytes, void* stream);
int opp_focal_loss_backward(const float* conf, const short* conf_gt, const float* weight, size_t n, float alpha,
                            float gamma, const float* scales, float* grad_conf, void* stream);

/* The same two passes on the ground truth AS THE CALLER HOLDS IT -- gt_kind 0 = int16, 1 = fp32 (the reference's dataset emits
 * float zeros / ones, OnePosePlus_dataset.py:174-236), 2 = uint8 / bool; values other than 0 / 1 are ignored -- and with the
 * weight of Loss.compute_c_weight (losses.py:103-111) formed on the fly from its two factors: mask0 [B * N] (per 3D point),
 * mask1 [B * L] (per image cell), weight[b][i][j] = mask0[b][i] * mask1[b][j]; n = B * N * L.  Pass `weight` (full array) OR
 * both masks OR neither.  No int16 copy of conf_gt and no B x N x L weight tensor is made. */
int opp_focal_loss_forward_ex(const float* conf, const void* conf_gt, int gt_kind, const float* weight, const float* mask0,
                              const float* mask1, int N, int L, size_t n, float alpha, float gamma, double* sums, void* workspace,
                              size_t workspace_bytes, void* stream);
int opp_focal_loss_backward_ex(const float* conf, const void* conf_gt, int gt_kind, const float* weight, const float* mask0,
                               const float* mask1, int N, int L, size_t n, float alpha, float gamma, const float* scales,
                               float* grad_conf, void* stream);

/* backward of conf = A * B, A = softmax(S, dim = points), B = softmax(S, dim = cells) (utils/coarse_matching.py:115);
 * sim, grad_conf, grad_sim [B][N][L]; lse_row [B][N] = logsumexp_j S_ij, lse_col [B][L] = logsumexp_i S_ij:
 *   grad_sim_ij = 2 conf_ij g_ij - A_ij sum_i' g_i'j conf_i'j - B_ij sum_j' g_ij' conf_ij'. */
size_t opp_dual_softmax_backward_workspace_bytes(int B, int N, int L);
int opp_dual_softmax_backward(const float* grad_conf, const float* sim, const float* lse_row, const float* lse_col,
                              int B, int N, int L, float* grad_sim, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ---- training step: backward of a bias-free nn.Linear (every Linear of loftr_coarse / loftr_fine,
 * loftr_module/transformer.py:26-47) on the MFMA GEMM.  Y [M][N] = X [M][K] W [N][K]^T (PyTorch layouts, fp32):
 *   grad_x [M][K] = grad_out [M][N] W            (NULL to skip; needs W)
 *   grad_w [N][K] = grad_out^T X                 (NULL to skip; needs X; accumulate_grad_w != 0 adds to the existing values):
 *                   a reduction over the M tokens, run as split-K with a fixed-order sum of the partials (deterministic).
 * N, K multiples of 32; prec 0 = exact-fp32 MFMA, 2 = bf16x3 (operands carried exactly, fp32 accumulate).  Both operands
 * are transposed / split into the workspace as needed; nothing is allocated. */
size_t opp_linear_backward_workspace_bytes(int M, int N, int K, int prec);
int opp_linear_backward(const float* grad_out, const float* X, const float* W, int M, int N, int K, float* grad_x, float* grad_w,
                        int accumulate_grad_w, int prec, void* workspace, size_t workspace_bytes, void* stream);

/* ---- training step: LinearAttention.forward with its backward (loftr_module/linear_attention.py:29-61) -------------------
 * Raw projections q [B][L][nhead][D], k, v [B][S][nhead][D] (fp32, contiguous; D = 32 or 16), optional masks q_mask [B][L],
 * kv_mask [B][S] (0 / 1 floats): out = (phi(q) KV) / (phi(q) . Ksum + 1e-6) * S with KV = sum_s phi(k_s)^T v_s / S,
 * phi = elu + 1.  forward also returns KV [B][nhead][D][D] and Ksum [B][nhead][D], which backward takes back together with
 * grad_out [B][L][nhead][D] and produces grad_q, grad_k, grad_v.  Token reductions are chunk partials summed in chunk order
 * (deterministic). */
size_t opp_linear_attention_train_workspace_bytes(int B, int L, int S, int nhead, int D);
int opp_linear_attention_train_forward(const float* q, const float* k, const float* v, const float* q_mask, const float* kv_mask, int B,
                                       int L, int S, int nhead, int D, float* out, float* kv, float* ks, void* workspace,
                                       size_t workspace_bytes, void* stream);
int opp_linear_attention_train_backward(const float* q, const float* k, const float* v, const float* q_mask, const float* kv_mask,
                                        const float* kv, const float* ks, const float* grad_out, int B, int L, int S, int nhead, int D,
                                        float* grad_q, float* grad_k, float* grad_v, void* workspace, size_t workspace_bytes,
                                        void* stream);

/* ---- training step: FullAttention.forward with its backward (loftr_module/linear_attention.py:64-95; no mask, no dropout) --
 * Raw projections q [B][L][nhead][D], k, v [B][S][nhead][D] (fp32, contiguous, 16-byte aligned): per head
 * out = softmax(q k^T / sqrt(D)) v.  forward also returns lse [B][nhead][L] = log2 sum_s 2^(logit_s log2 e) (BASE 2; x ln 2 = the
 * natural log-sum-exp of the scaled logits), which backward takes back together with out and grad_out [B][L][nhead][D]; it
 * rebuilds the probabilities tile by tile (nothing of size L x S is allocated; the workspace holds delta [B][nhead][L] =
 * sum_d grad_out out) and writes grad_q, grad_k, grad_v without atomics (bit-identical from call to call).
 * precision as opp_full_attention: 0 = fp32 MFMA, 3 = bf16x3; anything else OPP_ERR_UNSUPPORTED.  D = 32 with a stream longer
 * than 32 rows runs on MFMA kernels (csrc/full_attention_train.hip); shorter streams and D = 16 with both streams <= 64 rows on
 * exact-fp32 vector kernels in both precisions.  Every other shape (D = 16 with a longer stream, another D, B > 65535) returns
 * OPP_ERR_UNSUPPORTED before any launch, and the workspace size of such a shape is 0. */
size_t opp_full_attention_train_workspace_bytes(int B, int L, int S, int nhead, int D);
int opp_full_attention_train_forward(const float* q, const float* k, const float* v, int B, int L, int S, int nhead, int D, int precision,
                                     float* out, float* lse, void* workspace, size_t workspace_bytes, void* stream);
int opp_full_attention_train_backward(const float* q, const float* k, const float* v, const float* out, const float* lse,
                                      const float* grad_out, int B, int L, int S, int nhead, int D, int precision, float* grad_q,
                                      float* grad_k, float* grad_v, void* workspace, size_t workspace_bytes, void* stream);

/* ---- training step: ResNet-FPN forward that keeps its activations, and its backward ---------------------------------------
 * PL_OnePosePlus.training_step (src/lightning_model/OnePosePlus_lightning_model.py:54-81) differentiates the loss through
 * ResNetFPN_8_2.forward (backbone/resnet.py:141-164): nn.Conv2d (no bias), nn.BatchNorm2d in train(), ReLU / LeakyReLU(0.01),
 * the residual adds and the two bilinear x2 upsamples.  opp_backbone_train_tape is opp_backbone_train writing every tensor the
 * backward needs (raw convolution outputs, block outputs, batch mean / 1/sqrt(var + eps) per BatchNorm) into the caller's
 * `tape` (nothing is recomputed later) -- one walk serves both (csrc/api.hip: backbone_train_walk; the two entries differ in
 * where it writes: a slot of the tape each, or the reused maps of the workspace); opp_backbone_backward takes the gradients of
 * the two outputs, feat_c [B][H/8][W/8][256] and feat_f [B][H/2][W/2][128] (NHWC), and writes the gradient of EVERY backbone parameter: `weights` is the table given to
 * opp_pack_weights (the raw convolution weights are read from it), grads[i] the device pointer that receives the gradient of
 * weights[i] in the PyTorch layout ([cout][cin][kh][kw]; BatchNorm weight / bias [C]); entries of tensors outside the backbone
 * and of the running statistics are ignored and may be NULL.  Convolution input gradients run on the implicit-GEMM kernel with
 * the flipped / transposed weight, weight gradients on a pixel-major split reduction (csrc/conv_bwd.hip), in the arithmetic of
 * opp_config.gemm_precision (3 = bf16x3 or 0 = fp32; the weight-gradient kernel is bf16x3 in both: operands exact, fp32 accumulate). */
size_t opp_backbone_tape_bytes(const opp_ctx* ctx, int B, int H, int W);
size_t opp_backbone_train_tape_workspace_bytes(const opp_ctx* ctx, int B, int H, int W);
int opp_backbone_train_tape(opp_ctx* ctx, const float* image, int B, int H, int W, float* feat_c, float* feat_f, float* bn_stats,
                            void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream);
size_t opp_backbone_backward_workspace_bytes(const opp_ctx* ctx, int B, int H, int W);
int opp_backbone_backward(opp_ctx* ctx, const float* image, int B, int H, int W, const void* tape, size_t tape_bytes,
                          const float* const* weights, int n_weights, const float* grad_feat_c, const float* grad_feat_f,
                          float* const* grads, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of one nn.Conv2d (bias-free, kernel 1 or 3, padding k/2, stride 1 or 2; backbone/resnet.py:10-18) over NHWC tensors
 * whose channel counts are padded to multiples of 32 with zeros: x [B][Hin][Win][cin_pad], w [cout][cin][ks][ks] (PyTorch layout),
 * grad_y [B][Ho][Wo][cout_pad].  grad_x [B][Hin][Win][cin_pad] and / or grad_w [cout][cin][ks][ks] (either may be NULL);
 * grad_x_add (optional, same shape as grad_x, MAY ALIAS it) is added to the input gradient -- how the gradients of a tensor
 * with several consumers are accumulated.  prec 0 = fp32 MFMA, 2 = bf16x3. */
size_t opp_conv2d_backward_workspace_bytes(int B, int Hin, int Win, int cin, int cout, int ks, int stride, int prec);
int opp_conv2d_backward_nhwc(const float* x, int B, int Hin, int Win, int cin, const float* w, int cout, int ks, int stride,
                             const float* grad_y, float* grad_x, const float* grad_x_add, float* grad_w, int prec, void* workspace,
                             size_t workspace_bytes, void* stream);
/* Backward of nn.BatchNorm2d in train() followed by (+ residual) -> activation (backbone/resnet.py:25-26, :37-45) over an NHWC
 * tensor [rows][ld] with C real channels: y = act((raw - mean) * invstd * gamma + beta (+ res)); act 0 none, 1 ReLU, 2 LeakyReLU(0.01).
 * grad_y, y (unused for act 0), raw, the forward's batch mean / invstd [ld] in; grad_raw (may alias grad_y), grad_res (optional,
 * the residual branch's gradient; may alias grad_y), grad_gamma / grad_beta [C] (optional) out. */
size_t opp_batchnorm_backward_workspace_bytes(int rows, int ld);
int opp_batchnorm_backward_nhwc(const float* grad_y, const float* y, const float* raw, int rows, int ld, int C, int act,
                                const float* gamma, const float* mean, const float* invstd, float* grad_raw, float* grad_res,
                                float* grad_gamma, float* grad_beta, void* workspace, size_t workspace_bytes, void* stream);
/* Transpose of F.interpolate(scale_factor=2, mode='bilinear', align_corners=True) (backbone/resnet.py:151,155):
 * grad_in [B][Hr][Wr][ld] (+)= sum over the output pixels [B][2 Hr][2 Wr][ld] that read it. */
int opp_upsample2x_backward_nhwc(const float* grad_out, int B, int Hr, int Wr, int ld, float* grad_in, int accumulate, void* stream);
/* nn.LayerNorm (eps 1e-5) over rows of C = 64 / 128 / 256 values with the statistics kept for the backward
 * (loftr_module/transformer.py:87-88, :92-94): y = (residual ? residual : 0) + LN(x) * gamma + beta; mean / rstd [rows] out.
 * backward: grad_x [rows][C], grad_gamma / grad_beta [C] (fixed-order reduction over the rows). */
int opp_layer_norm_train_forward(const float* x, const float* gamma, const float* beta, const float* residual, int rows, int C,
                                 float* y, float* mean, float* rstd, void* stream);
size_t opp_layer_norm_train_backward_workspace_bytes(int rows, int C);
int opp_layer_norm_train_backward(const float* grad_y, const float* x, const float* gamma, const float* mean, const float* rstd,
                                  int rows, int C, float* grad_x, float* grad_gamma, float* grad_beta, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* Dual softmax of the score matrix sim [B][N][L] (utils/coarse_matching.py:115) with what opp_dual_softmax_backward needs:
 * lse_row [B][N] = logsumexp over the cells, lse_col [B][L] = logsumexp over the points; conf (optional, may alias sim) =
 * exp(sim - lse_col) * exp(sim - lse_row). */
size_t opp_dual_softmax_forward_workspace_bytes(int B, int N, int L);
int opp_dual_softmax_forward(const float* sim, int B, int N, int L, float* lse_row, float* lse_col, float* conf, void* workspace,
                             size_t workspace_bytes, void* stream);
/* FinePreprocess on a batch (loftr_module/fine_preprocess.py:41-55: F.unfold + [b_ids, j_ids] indexing): windows [M][W*W][C] from
 * feat_f [B][Hf][Wf][C] around coarse cell j_ids[m] of image b_ids[m] (zeros outside the image); the backward adds the windows'
 * gradients into grad_feat_f (zeroed first; overlapping windows are summed with fp32 atomics). */
int opp_fine_window_gather(const float* feat_f, int B, int Hf, int Wf, int C, const long long* b_ids, const long long* j_ids,
                           int n_matches, int hc, int wc, int window, float* windows, void* stream);
int opp_fine_window_gather_backward(const float* grad_windows, int B, int Hf, int Wf, int C, const long long* b_ids,
                                    const long long* j_ids, int n_matches, int hc, int wc, int window, float* grad_feat_f,
                                    void* stream);

/* FineMatching's expectation head on its own (utils/fine_matching.py:63-94: heatmap = softmax(<f3, win_r> / sqrt(C)), spatial expectation and
 * the summed standard deviation) for the training graph, and its backward.  f3 [M][C] point tokens, win [M][window^2][C] window tokens, expec_f
 * [M][3]; scratch_xy: 4 M floats.  Backward: grad_expec_f [M][3] -> grad_f3 [M][C], grad_win [M][window^2][C] (every element written). */
int opp_fine_head_train_forward(const float* f3, const float* win, int n_matches, int window, int C, float* expec_f, float* scratch_xy,
                                void* stream);
int opp_fine_head_train_backward(const float* f3, const float* win, int n_matches, int window, int C, const float* grad_expec_f,
                                 float* grad_f3, float* grad_win, void* stream);

/* Ground-truth matrices of one training sample, formed on the device from the k assignment pairs
 * (OnePosePlusDataset.build_assignmatrix, src/datasets/OnePosePlus_dataset.py:174-236; the loader builds 229 MB per sample on the host
 * at N = 7000).  kp2d_coarse / kp2d_fine [n2d][2] fp32; assign [2][k] int64 (row 0: 2D keypoint index, row 1: padded 3D point index);
 * scale_x / scale_y = query_img_scale[1] / [0].  conf_gt [N][L] int16 (zeroed here, 1 at the pairs), fine_loc_gt [N][L][2] fp32 (-50
 * filled here, the fine keypoint at the pairs; 16-byte aligned); pairs with a 3D index >= N or j > L are dropped like upstream, of
 * duplicate (i, j) pairs the last one wins (CPU index_put).  keys: k int64 of scratch.  *status (device int): bit 0 = an index upstream
 * raises IndexError on (skipped here), bit 1 = duplicate pairs seen (upstream logs "Keypoints duplicate!"). */
int opp_build_assignmatrix(const float* kp2d_coarse, const float* kp2d_fine, int n2d, const long long* assign, int k, int N, int L,
                           int w_c, float scale_x, float scale_y, float coarse_scale, short* conf_gt, float* fine_loc_gt,
                           long long* keys, int* status, void* stream);

/* ---- a training sample's tensors from its annotation arrays (the training branch of OnePosePlusDataset.read_anno,
 * src/datasets/OnePosePlus_dataset.py:341-437, in front of opp_build_assignmatrix; csrc/train_sample.hip) ----------------
 * kornia 0.4.1's homography_warp of B fp32 images [B][1][h][w] in one launch (restated: kornia is not pinned in this project).  src: rows
 * src_stride floats apart, images src_batch_stride floats apart; src_homo_dst [B][3][3] row-major fp32 ON THE DEVICE, the NORMALISED matrix
 * the reference passes (the inverse of normalize_homography(H)); dst [B][h][w] dense.  Destination grid linspace(-1, 1, w) x
 * linspace(-1, 1, h); transform_points with scale 1 / z where |z| > 1e-8, else 1; grid_sample(bilinear, zeros, align_corners).  The identity
 * with align_corners != 0 returns the input bit for bit.  h, w >= 2. */
int opp_homography_warp(const float* src, int B, int h, int w, int src_stride, long long src_batch_stride, const float* src_homo_dst,
                        int align_corners, float* dst, void* stream);
/* mkpts_proj [k][2] fp32: pair t's 3D point keypoints3d[assign[1][t]] ([n3d][3] fp32, assign [2][k] int64, both on the device) through
 * K (R X + t) with x / (z + 1e-6), then -- homography_px != NULL -- through that pixel-space homography with the division by its third row.
 * pose_Rt [3][4], K [3][3], homography_px [3][3]: row-major fp32 in HOST memory, read before the call returns.  Arithmetic in double from the
 * fp32 inputs.  A 3D index out of range gives NaN and ORs bit 0 into *status (device int, may be NULL; not zeroed here). */
int opp_project_pairs(const float* keypoints3d, int n3d, const long long* assign, int k, const float* pose_Rt, const float* K,
                      const float* homography_px, float* mkpts_proj, int* status, void* stream);
/* The pairs that survive read_anno's filters, exactly (:393-433): warped != 0 drops unrounded points < 0, > w - 1, > h - 1; then
 * r = round_half_even(p / cell) * cell in fp32 and the same bounds on r; of the pairs with one r (-0.0 = 0.0) the smallest index stays; the
 * survivors are ordered by (r.x, r.y) as np.unique(axis=0) orders them.  assign_out [2][k] int64 (row stride k): the k' survivors'
 * columns, then k - k' columns (0, INT64_MAX) that opp_build_assignmatrix drops silently -- so it takes assign_out with the same k and no
 * host round trip; *n_out = k' (device int).  kp2d_coarse / kp2d_fine [n2d][2] fp32: rows assign_out[0][:k'] receive r / p, the last
 * survivor in that order where a 2D index repeats; other rows are untouched (upstream: the input coarse keypoints / zeros).  scratch:
 * (h / cell + 1) (w / cell + 1) + n2d ints.  *status (device int, may be NULL, not zeroed here): bit 0 = a non-finite point or a 2D index
 * out of range (upstream raises).  h, w multiples of cell.  One workgroup; deterministic. */
int opp_select_pairs(const float* mkpts_proj, const long long* assign, int k, int h, int w, int cell, int warped, int n2d,
                     float* kp2d_coarse, float* kp2d_fine, long long* assign_out, int* n_out, int* scratch, int* status, void* stream);

/* ---- building blocks (exported for stage-level parity tests and tuning) ------------------ */
/* NHWC convolution as implicit GEMM on the MFMA.  x [Hin][Win][cin_pad], cin_pad = cin rounded up to 32 (pad
 * channels zero); w_packed [cout_pad][opp_conv_packed_k(cin, ks)] (from opp_pack_conv_weight with the same cin:
 * ks*ks*cin_pad, or the shorter K-tail packing for a 3x3 kernel over 32 n + (1..4) channels); bias [cout_pad] or NULL; residual:
 * res_mode 0 none, 1 same-shape NHWC [Hout][Wout][cout_pad], 2 bilinear x2 (align_corners)
 * upsample of NHWC [Hout/2][Wout/2][cout_pad]; act 0 none, 1 ReLU, 2 LeakyReLU(0.01).
 * tile_cfg < 0 selects automatically (an explicit 27 -- the 128x224 tile -- treats weight rows >= 208 as the zero padding they are for a
 * 196-channel layer: the caller vouches for it).  prec = operand arithmetic: 0 fp32; 1 fp16x2 (w_packed additionally
 * pre-split by opp_pack_h2, h2_scale = the scale2 pointer given to it, or NULL); 2 bf16x3 (w_packed pre-split by
 * opp_pack_b3, 1.5x the floats). */
int opp_conv2d_nhwc(const float* x, int Hin, int Win, int cin, const float* w_packed,
                    const float* bias, int cout_pad, int ks, int stride, const float* residual,
                    int res_mode, int act, float* y, int tile_cfg, int prec, const float* h2_scale,
                    void* stream);
/* The same convolution in the bf16x3 arithmetic with PRE-SPLIT activations (round 6; what the inference backbone chains its layers with --
 * nn.Conv2d + BatchNorm2d + activation of backbone/resnet.py:10-45, :141-164 -- so that a map is split into bf16 triples once, by the
 * epilogue that produces it, instead of in the K loop of every tap and column tile that reads it).  A pre-split map holds, per pixel row,
 * every 8 channels as 48 bytes [hi x8 | mid x8 | lo x8] (bf16; opp_pack_b3 over the fp32 rows gives exactly these bytes), 6 cin_pad bytes
 * per pixel, 16-byte aligned.  x_split != NULL: the input is read from it when the convolution's K walk has no packed tail (any 1x1; 3x3
 * over cin % 32 == 0 real channels), else from x (one of the two must serve).  y_split != NULL: the epilogue also writes the output
 * pre-split (y may then be NULL).  Results are bit-identical to opp_conv2d_nhwc(prec = 2). */
int opp_conv2d_nhwc_split(const float* x, const void* x_split, int Hin, int Win, int cin, const float* w_packed,
                          const float* bias, int cout_pad, int ks, int stride, const float* residual, int res_mode,
                          int act, float* y, void* y_split, int tile_cfg, void* stream);
int opp_pack_conv_weight(const float* w, const float* scale, int cout, int cin, int ks,
                         int cout_pad, int cin_pad, float* out, void* stream);
/* floats per packed weight row of a (cin, ks) convolution */
int opp_conv_packed_k(int cin, int ks);
/* LinearAttention (loftr_module/linear_attention.py:29-61) of the two token streams of one encoder layer, as the
 * transformer runs it.  qkv [n_seg * (len0 + len1)][3 C]: per row phi(Q) | phi(K) | V / S (phi = elu + 1, S = the
 * row's own stream length; the QKV GEMM epilogue produces exactly this), the n_seg segments of stream 0 (len0 rows
 * each) first, then those of stream 1 (len1 rows each).  msg [same rows][C] = phi(Q) (sum_s phi(K_s)^T V_s / S)
 * / (phi(Q) . sum_s phi(K_s) + 1e-6) * S_src; cross = 0: every stream attends to itself, 1: to the other stream's
 * K, V of the same segment.  Supported: (C, nhead) = (256, 8) and (128, 8). */
size_t opp_linear_attention_workspace_bytes(int n_seg, int len0, int len1, int C, int nhead);
int opp_linear_attention(const float* qkv, int n_seg, int len0, int len1, int C, int nhead, int cross,
                         float* msg, void* workspace, size_t workspace_bytes, void* stream);
/* FullAttention (loftr_module/linear_attention.py:64-95, selected by transformer.py:32-40 for any `attention` but "linear") of the
 * two token streams of one encoder layer, same row layout as opp_linear_attention but qkv holds the PLAIN projections Q | K | V.
 * Per head (D = C / nhead): msg = softmax(Q K^T / sqrt(D)) V over the source tokens of the same segment (cross = 0: the row's own
 * stream, 1: the other stream); no mask, no dropout.  precision = opp_config.gemm_precision: 0 fp32 MFMA, 3 bf16x3 (six bf16 MFMAs per
 * product, not narrower than fp32); other values return OPP_ERR_UNSUPPORTED.  D = 32 with a stream longer than 32 rows runs the flash
 * kernel (online softmax, K / V tiles through LDS), everything else (the fine level: 25 + 1 tokens, D = 16) an exact-fp32 vector-ALU
 * kernel.  Supported: len0, len1 >= 1, C % nhead == 0, D in {16, 32}.  Needs no workspace (the size query returns 0; ws may be NULL). */
size_t opp_full_attention_workspace_bytes(int n_seg, int len0, int len1, int C, int nhead);
int opp_full_attention(const float* qkv, int n_seg, int len0, int len1, int C, int nhead, int cross, int precision,
                       float* msg, void* workspace, size_t workspace_bytes, void* stream);
/* The tile configuration the GEMM / implicit-GEMM convolution launcher picks by itself (tile_cfg < 0) for an M x n_store output over K (a multiple
 * of 32) -- a pure host function of shape, operand arithmetic (prec as in opp_conv2d_nhwc) and tile policy (0 latency, 1 throughput: opp_config.tile_policy),
 * exported so that the policy is testable without a device.  n_real = real output channels when n_store is their padded count (0 = unknown), conv != 0
 * for a convolution.  Returns the tile config (the list under opp_profile_start), + 1000 when a bf16x3 convolution of this shape runs as four K slices
 * on that tile, or a negative OPP_ERR_*.  Replaces nothing in the reference (cuDNN / cuBLAS pick their own kernels: backbone/resnet.py:10-45). */
int opp_gemm_tile_for(int M, int n_real, int n_store, int K, int conv, int prec, int tile_policy);

/* C[M][N] = act(A[M][K] * W[N][K]^T) ; act 0 none, 1 ReLU.  prec as above (1: W pre-split by opp_pack_h2,
 * 2: by opp_pack_b3). */
int opp_linear(const float* A, int M, int K, const float* W, int N, int act, float* C,
               int tile_cfg, int prec, const float* h2_scale, void* stream);
/* fp16x2 pre-split of a K-contiguous weight matrix (n floats, n % 8 == 0, out != in, same size).
 * scale2 (device, 2 floats, may be NULL): receives {s, 1/s}, s the power of two that brings max|w|
 * into [2^14, 2^15) and is applied before the split; pass the same pointer as h2_scale to
 * opp_linear / opp_conv2d_nhwc, which multiply the accumulators by 1/s (exact). */
int opp_pack_h2(const float* in, float* out, size_t n, float* scale2, void* stream);
/* bf16x3 pre-split of a K-contiguous operand (n floats, n % 8 == 0, out != in): out receives 1.5 n floats, every
 * 8 consecutive values as 48 bytes [hi x8 | mid x8 | lo x8] bf16 with hi + mid + lo == x exactly. */
int opp_pack_b3(const float* in, float* out, size_t n, void* stream);
/* C[M][N] = (residual ? residual : 0) + LayerNorm_N(A[M][K] * W[N][K]^T) * gamma + beta, N in {256, 128}:
 * the LayerNorm (eps 1e-5) runs in the GEMM epilogue (merge -> norm1, mlp.2 -> norm2 -> +x of
 * LoFTREncoderLayer.forward, loftr_module/transformer.py:86-94).  residual may alias C. */
int opp_linear_layernorm(const float* A, int M, int K, const float* W, int N, const float* gamma,
                         const float* beta, const float* residual, float* C, int prec,
                         const float* h2_scale, void* stream);
int opp_layer_norm(const float* x, const float* gamma, const float* beta, const float* residual,
                   float* out, int rows, int C, void* stream);

/* ---- query-image ingest ------------------------------------------------------
 * 8-bit grayscale frame [h][src_stride] on the device -> cv2.resize(INTER_LINEAR, 8-bit fixed point)
 * to [h_new][w_new] -> fp32 / 255 (read_grayscale + grayscale2tensor, src/utils/data_io.py:34-69,
 * :105-106).  dst (fp32, row stride dst_stride floats; e.g. a pad_to canvas) and dst_u8 (the resized
 * 8-bit image, packed) are both optional, at least one must be given. */
int opp_image_ingest_u8(const unsigned char* src, int h, int w, int src_stride, int h_new, int w_new,
                        float* dst, int dst_stride, unsigned char* dst_u8, void* stream);

/* ---- tracking crop (demo.py:98-134) --------------------------------------------------------------
 * n_boxes crops of one 8-bit grayscale frame [h][src_stride] on the device, each crop_size x crop_size:
 * crop_img_by_bbox (local_feature_2D_detector.py:133-159) = two cv2.warpAffine(INTER_LINEAR, constant
 * border 0) -- the window [x0, y0, x1, y1] copied with zeros outside the frame, then scaled by
 * crop_size / (x1 - x0) about its centre (a box that is not square is cut or zero-padded vertically) --
 * as 8-bit fixed point, then fp32 / 255.  boxes: int32 [n_boxes][4] on the DEVICE, read by the kernel;
 * boxes_host: the same values on the host, checked before the launch.  Refused without any launch:
 * crop_size not a power of two in [64, 1024], an empty box (x1 - x0 < 1 or y1 - y0 < 1), a frame side
 * or box coordinate at or beyond 32767.  No tap reads outside the frame, whatever the boxes hold.
 * dst (fp32 [n_boxes][crop_size][crop_size]) and dst_u8 (the same crops as 8-bit values) are both
 * optional, at least one must be given. */
int opp_crop_warp_u8(const unsigned char* src, int h, int w, int src_stride, const int* boxes,
                     const int* boxes_host, int n_boxes, int crop_size, float* dst, unsigned char* dst_u8,
                     void* stream);

/* ---- per-object descriptor bank (the step before the path) ----------------------
 * mean_descriptors_and_scores (src/sfm_utils/postprocess/feature_process.py:527-541): out[i][:] = mean over rows
 * [offsets[i], offsets[i+1]) of `rows` [R][D] fp32 (the 2D features of the track of 3D point i, concatenated in
 * track order by gather_3d_ann, :255-311); float32 row-by-row accumulation and float32 division like numpy's
 * axis-0 mean, i.e. bit-identical to the reference.  offsets: n_seg + 1 int64 on the device. */
int opp_segmented_mean(const float* rows, int D, const long long* offsets, int n_seg, float* out, void* stream);

/* ---- SfM point cloud post-processing: what runs between COLMAP's points3D and the bank above ----------------
 * filter_bbox and merge of src/sfm_utils/postprocess/filter_points.py (:172-234, :265-297) in float64, every
 * operation rounded on its own (no FMA contraction).  xyz [n][3] float64 on the device, n <= 2^20.
 *
 * opp_pc_box_mask: mask[i] = 1 iff 0 < (p - c4) . v < v . v for v = c5 - c4, c0 - c4, c7 - c4 (strict on every
 * face).  `corners` [8][3] is a HOST array. */
int opp_pc_box_mask(const double* xyz, int n, const double* corners, unsigned char* mask, void* stream);
/* The merge, in five steps the caller strings together (onepose_plus_plus_amd/pointcloud.py); nothing of size n x n
 * is ever allocated.  N(j) = { i : sqrt(dx^2 + dy^2 + dz^2) < thr }, j itself included.
 *   1. opp_pc_neighbor_count: counts[j] = |N(j)| (int32 [n]).
 *   2. the caller forms offsets [n + 1] int64 = exclusive prefix sum of counts and reads pairs = offsets[n] back;
 *      it refuses a total above its own limit here, before the lists are allocated.
 *   3. opp_pc_neighbor_fill: N(j) in ascending index at nbr[offsets[j] .. offsets[j + 1]) inside the workspace.
 *   4. opp_pc_select: sel[j] = 1 iff the reference's walk j = 0 .. n-1 takes row j (no earlier taken row shares a
 *      neighbour with it); selcnt[j] = sel[j] ? |N(j)| : 0.  One workgroup iterates rounds, at most n; *status = 1
 *      if that bound was reached with rows undecided (the results are then invalid), else 0.
 *   5. opp_pc_emit: rank / mem_end [n] int64 = INCLUSIVE prefix sums of sel / selcnt, n_clusters / n_members their
 *      last entries.  Cluster c = the c-th selected row: ret_points[c] = ((x_i0 + x_i1) + ...) / k over N(j) in
 *      ascending position (numpy's axis-0 mean), members[cl_offsets[c] .. cl_offsets[c + 1]) = ids[N(j)].
 * opp_pc_workspace_bytes is host-only; the same workspace (and `pairs`) goes to steps 3-5.  0 = arguments out of range. */
size_t opp_pc_workspace_bytes(int n, long long pairs);
int opp_pc_neighbor_count(const double* xyz, int n, double thr, int* counts, void* stream);
int opp_pc_neighbor_fill(const double* xyz, int n, double thr, const long long* offsets, long long pairs, void* ws, size_t ws_bytes,
                         void* stream);
int opp_pc_select(const long long* offsets, int n, long long pairs, int* sel, int* selcnt, int* status, void* ws, size_t ws_bytes,
                  void* stream);
int opp_pc_emit(const double* xyz, const long long* ids, int n, long long pairs, const long long* offsets, const int* sel,
                const long long* rank, const long long* mem_end, long long n_clusters, long long n_members, double* ret_points,
                long long* cl_offsets, long long* members, void* ws, size_t ws_bytes, void* stream);

/* ---- pose from the matches (next row after the matcher) --------------------
 * PnP-RANSAC on the device: replaces ransac_PnP / cv2.solvePnPRansac(EPNP, 10000 iterations)
 * (src/utils/metric_utils.py:121-204) so the matches never leave the GPU.  pts2d [n][2] (pixels),
 * pts3d [n][3] fp32 on the device; K4 = {fx, fy, cx, cy} on the HOST; `scale` multiplies the 3D
 * points before solving and divides the translation after (reference `point_cloud_rescale`).
 * Outputs on the device: pose_out [12] doubles = row-major [R | t] (3x4), inlier_mask [n] (0/1),
 * n_inliers, ok (0 -> identity pose, the reference's cv2.error branch).  Deterministic for a seed.
 * Fewer than 4 matches give that failure result; with n_points == 0 pts2d and pts3d may be NULL (an
 * empty tensor has no address) and inlier_mask is not written, as in opp_pnp_ransac_ex. */
size_t opp_pnp_workspace_bytes(int iterations);
int opp_pnp_ransac(const float* pts2d, const float* pts3d, int n_points, const double* K4,
                   double reproj_error_px, double scale, int iterations, unsigned seed,
                   int refine_iters, double* pose_out, int* inlier_mask, int* n_inliers, int* ok,
                   void* workspace, size_t workspace_bytes, void* stream);
/* The same with a choice of minimal solver and OpenCV's adaptive stop.  solver 0 = P3P + Gauss-Newton (opp_pnp_ransac;
 * identical to it when confidence >= 1), 1 = EPnP as in cv2.solvePnPRansac(flags=SOLVEPNP_EPNP): 5-match EPnP hypotheses
 * (P3P when n == 4, one EPnP solve on all points when n == 5), an EPnP refit on the best hypothesis's RANSAC inliers, which
 * are the inliers returned (refine_iters is ignored).  confidence (OpenCV default 0.99; >= 1: never stop early) sets
 * niters = RANSACUpdateNumIters after each new best; the result is that of the sequential loop over hypotheses 0, 1, ...
 * Extra device outputs: stop_out (1 int: hypotheses the sequential loop evaluates), and, when not NULL, samples_out
 * [iterations][5] (sample indices; -1 in the 5th column for P3P) and scores_out [iterations] (inlier counts, -1 = no model),
 * written whenever hypotheses are drawn (n >= 4; with solver 1 not for n == 5).
 * Workspaces: the three P3P / EPnP entries share one layout (opp_pnp_layout, csrc/pnp_batch.h): per sample the hypotheses, their
 * validity, the scores and the scores masked past the stop index, then 13 doubles per match for the refit.  This entry's is
 * the batch's at n_samples = 1; opp_pnp_ransac's is its leading part (no masked scores, no refit). */
size_t opp_pnp_ex_workspace_bytes(int iterations, int n_points);
int opp_pnp_ransac_ex(const float* pts2d, const float* pts3d, int n_points, const double* K4,
                      double reproj_error_px, double scale, int iterations, unsigned seed,
                      int refine_iters, int solver, double confidence, double* pose_out, int* inlier_mask,
                      int* n_inliers, int* ok, int* stop_out, int* samples_out, int* scores_out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* opp_pnp_ransac_ex for a whole batch in one enqueue, with no device-to-host copy and no host decision on a sample's size.
 * The matches of the n_samples (1..1024) samples lie concatenated in sample order: pts2d [n_total][2], pts3d [n_total][3];
 * offsets [n_samples + 1] (device) delimits them, so sample b has offsets[b+1] - offsets[b] matches, a number the host need
 * not know (a pair of offsets that is no segment of [0, n_total] makes an empty sample).  K4 [n_samples][4] and seeds
 * [n_samples] are DEVICE arrays; the threshold, scale, iterations, solver and confidence hold for every sample.  Outputs on
 * the device: pose_out [n_samples][12], inlier_mask [n_total] (0/1, indexed like the matches), n_inliers, ok and stop
 * [n_samples].  Sample b's outputs are bit for bit those of opp_pnp_ransac_ex on its slice with K4[b] and seeds[b]; a failed
 * sample (fewer than 4 matches, no model) gets the identity pose, a zeroed mask segment, ok = 0, n_inliers = 0.  n_total = 0
 * is legal (every sample fails).
 * opp_pnp_offsets makes `offsets` from the matcher's batch ids m_bids [n_total] (int64, non-decreasing, in [0, n_samples),
 * as the coarse matcher's ordered compaction emits them) by a lower-bound search per boundary; *bad (device) becomes 1 when
 * the ids break that contract and 0 otherwise. */
size_t opp_pnp_batch_workspace_bytes(int iterations, int n_samples, int n_total);
int opp_pnp_offsets(const long long* m_bids, int n_total, int n_samples, int* offsets, int* bad, void* stream);
int opp_pnp_ransac_batch(const float* pts2d, const float* pts3d, const int* offsets, int n_samples, int n_total,
                         const double* K4, const unsigned* seeds, double reproj_error_px, double scale, int iterations,
                         int refine_iters, int solver, double confidence, double* pose_out, int* inlier_mask,
                         int* n_inliers, int* ok, int* stop, void* workspace, size_t workspace_bytes, void* stream);

/* LO-RANSAC with robust refinement: the reference's pycolmap branch (pycolmap.absolute_pose_estimation, i.e. COLMAP 3.8
 * EstimateAbsolutePose: LORANSAC<P3PEstimator, EPNPEstimator>, then RefineAbsolutePose under a Cauchy loss).  Trial t draws 3
 * matches (the sampler of opp_pnp_ransac), P3P gives 0..4 models and every one is scored: support = (inliers, sum of their
 * squared reprojection errors), inlier = error <= reproj_error_px^2 in front of the camera, better = more inliers or as many and a
 * smaller sum.  A model that beats the best support with more than 4 inliers is locally optimised (EPnP on the best model's
 * inliers, repeated while the inlier count grows, at most 10 times).  After every new best dyn = ceil(3 log(1 - confidence) /
 * log(1 - r^3)), r = inliers / n; the loop ends at the first trial >= dyn and >= min_trials, `iterations` at the latest
 * (confidence >= 1: never earlier).  The best model's inliers are the ones returned; the pose is refined on them by
 * Levenberg-Marquardt on sum log(1 + error) (a step is taken only when that cost falls, <= 100 iterations, stop at
 * |gradient|_inf <= 1).  The points are not rescaled; K4 =
 * {fx, fy, cx, cy} on the host (the reference's SIMPLE_PINHOLE camera: pass fy = fx).  Failure (identity pose, ok = 0, empty mask):
 * n < 3, no model, or a best inlier count of 0 or below min_inlier_ratio * n.  All trials run in parallel; the result is that of the
 * sequential loop.  stop_out (may be NULL): trials the sequential loop runs.  `record` (may be NULL, any member may be NULL):
 * device buffers for what the run decided on; entries of trials past the stop bound are left as they were. */
typedef struct OppLoRecord {
  int* samples;        /* [iterations][3] match indices of every trial */
  int* counts;         /* [iterations][4] inliers of every model, -1 = no such model */
  double* sums;        /* [iterations][4] residual sum of its inliers */
  double* models;      /* [iterations][4][12] the models, row-major [R | t] as 9 + 3 */
  int* n_cand;         /* 1: models whose support beats every earlier model's (the only ones LO can run on) */
  int* cand_idx;       /* [iterations * 4] 4 * trial + model of each, ascending */
  int* cand_cnt;       /* [iterations * 4] support after local optimisation */
  double* cand_sum;
  int* cand_taken;     /* [iterations * 4] 1 = became the best in the sequential loop; the last one taken is the result */
  double* ransac_pose; /* [12] row-major 3x4 pose before the refinement */
  int* lm_iters;       /* 1: damped systems the refinement solved */
} OppLoRecord;
size_t opp_pnp_loransac_workspace_bytes(int iterations, int n_points);
int opp_pnp_loransac(const float* pts2d, const float* pts3d, int n_points, const double* K4,
                     double reproj_error_px, int iterations, unsigned seed, double confidence, int min_trials,
                     double min_inlier_ratio, double* pose_out, int* inlier_mask, int* n_inliers, int* ok,
                     int* stop_out, const OppLoRecord* record, void* workspace, size_t workspace_bytes, void* stream);

/* opp_pnp_loransac for a whole batch in one enqueue, with no device-to-host copy and no host decision on a sample's size: the
 * batch conventions of opp_pnp_ransac_batch (matches concatenated in sample order, `offsets` [n_samples + 1], K4 [n_samples][4]
 * and seeds [n_samples] DEVICE arrays, a pair of offsets that is no segment of [0, n_total] makes an empty sample; offsets from
 * opp_pnp_offsets).  The threshold, iterations, confidence, min_trials and min_inlier_ratio hold for every sample.  Outputs on
 * the device: pose_out [n_samples][12], inlier_mask [n_total] (0/1, indexed like the matches), n_inliers, ok and stop
 * [n_samples]; every entry is written.  Sample b's outputs are bit for bit those of opp_pnp_loransac on its slice with K4[b]
 * and seeds[b]; a failed sample (fewer than 3 matches, no model, too few inliers) gets the identity pose, a zeroed mask segment,
 * ok = 0, n_inliers = 0 (and stop = 0 with fewer than 3 matches).  n_total = 0 is legal (every sample fails).  A focal length
 * <= 0 cannot be refused here (K4 is on the device): the caller checks it.  There are no record outputs.  The workspace holds
 * about 948 * iterations bytes per sample plus 3496 bytes per match (opp_lo_batch_layout, csrc/pnp_lo_batch.h; opp_pnp_loransac's
 * is the same layout at n_samples = 1); one that is too small is refused before any launch. */
size_t opp_pnp_loransac_batch_workspace_bytes(int iterations, int n_samples, int n_total);
int opp_pnp_loransac_batch(const float* pts2d, const float* pts3d, const int* offsets, int n_samples, int n_total,
                           const double* K4, const unsigned* seeds, double reproj_error_px, int iterations,
                           double confidence, int min_trials, double min_inlier_ratio, double* pose_out,
                           int* inlier_mask, int* n_inliers, int* ok, int* stop, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- 2D box by matches: affine RANSAC for a batch of views (the estimator half of the reference's first-frame detector,
 * src/local_feature_object_detector/local_feature_2D_detector.py:74-131) ------------------------------------------------------
 * cv2.estimateAffine2D(method = RANSAC) for n_views (1..1024) views in one enqueue, as we read OpenCV 4.x (its source is not
 * available here: parity unpinned), then the box of each view's image corners under its map and the box of the view with the
 * most inliers.  The batch conventions are those of opp_pnp_ransac_batch: pts0 [n_total][2] (the view's image) and pts1
 * [n_total][2] (the query frame) hold the matches of all views concatenated in view order, `offsets` [n_views + 1] (device;
 * opp_pnp_offsets makes it from per-match view ids) delimits them, a pair of offsets that is no segment of [0, n_total] makes an
 * empty view, seeds [n_views] is a device array.  corners [n_views][4][2] (device, doubles): the points mapped into the box, the
 * reference's (0,0), (W,0), (0,H), (W,H) of each view's image.  fallback_box: four ints on the HOST, the box of a view without a
 * model (the reference's image centre +- 500).
 * Per view, with n matches: hypothesis h draws 3 distinct matches from the hash sampler of opp_pnp_ransac (n == 3: one hypothesis
 * on matches 0, 1, 2); a sample whose SOURCE points are collinear by OpenCV's haveCollinearPoints test scores -1 and still counts
 * as an iteration (OpenCV draws again); the 2 x 3 map is solved in closed form in float64; a match is an inlier when the squared
 * distance of its mapped source point to its query point is <= thr_px^2; a new best needs more than max(best, 2) inliers and
 * OpenCV's adaptive stop runs at `confidence` (>= 1: never), the stop index and best hypothesis being those of the sequential loop
 * over h = 0, 1, ...; the inliers returned are those of the best hypothesis; with `refine` and more than 3 of them the map is the
 * linear least-squares fit on the inliers, solved in coordinates centred on their mean (OpenCV runs 10 Levenberg-Marquardt
 * iterations on this linear problem: the same minimiser).  The four corners are mapped, truncated towards zero to int32, and
 * box = min x, min y, max x, max y.
 * Outputs on the device, every entry written: affine_out [n_views][6] (row-major 2 x 3), inlier_mask [n_total] (0/1, indexed like
 * the matches; 0 for a match no view covers), n_inliers, ok, stop [n_views], boxes [n_views][4], best_view [1] (the ok view with
 * the most inliers, the first on ties; -1 when there is none) and best_box [4] (its box, or the fallback box).  A failed view
 * (fewer than 3 matches, no hypothesis above 2 inliers, a mapped corner that is not finite or does not fit int32) gets the
 * identity map, a zeroed mask segment, n_inliers = 0, ok = 0 and the fallback box; stop = 0 with fewer than 3 matches.
 * samples_out [n_views][iterations][3] and scores_out [n_views][iterations] may be NULL; hypotheses a view does not evaluate
 * are recorded as -1.  View v's outputs are bit for bit those of a call on its slice alone with seeds[v].  n_total = 0 is legal
 * (every view fails).  The workspace (opp_affine_layout, csrc/affine_batch.h) holds 60 bytes per hypothesis and view. */
size_t opp_affine2d_batch_workspace_bytes(int iterations, int n_views, int n_total);
int opp_affine2d_ransac_batch(const float* pts0, const float* pts1, const int* offsets, int n_views, int n_total,
                              const unsigned* seeds, const double* corners, double thr_px, int iterations,
                              double confidence, int refine, const int* fallback_box,
                              double* affine_out /* [n_views][6] row-major 2x3 */, int* inlier_mask /* [n_total] */,
                              int* n_inliers, int* ok, int* stop, int* boxes /* [n_views][4] */,
                              int* best_view /* [1] */, int* best_box /* [4] */,
                              int* samples_out /* [n_views][iterations][3] or NULL */,
                              int* scores_out /* [n_views][iterations] or NULL */,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- pose-error metrics (the scoring half of compute_query_pose_errors, src/utils/metric_utils.py:207-292) --------
 * Scores n_poses poses of ONE model in a single enqueue (at most three launches, no host synchronisation, no allocation):
 * query_pose_error (:91-118), add_metric's mean distance (:55-87; ADD, or ADD-S = for every TARGET point the nearest PREDICTED
 * point, as cKDTree(model_pred).query(model_target) does) and projection_2d_error (:31-53; divides by z, no guard).  All fp64.
 * Device pointers: model_pts [n_points][3] fp32 (NULL with n_points = 0: only the 3x3 / translation metrics); pose_pred, pose_gt
 * [n_poses][12] row-major 3x4 R | t; K [n_poses][9] row-major, or NULL = no 2D error; syn [n_poses] 0 = ADD, 1 = ADD-S, or NULL =
 * all 0 (the ADD-S sweep is then not launched); valid [n_poses] 0 = failed pose, or NULL = all valid.  t_to_cm: 100 for models in
 * 'm', 1 for 'cm', 0.1 for 'mm'.  out [n_poses][4] = rotation error (degrees; trace clamped from above only, as upstream),
 * translation error (cm), mean distance (model units), mean 2D error (pixels; NaN without K, both NaN without points); a row with
 * valid = 0 is +inf four times.  Results are bit-identical from run to run (fixed-order sums, no atomics).  A workspace smaller
 * than opp_pose_metrics_workspace_bytes(n_poses, n_points) is refused before any launch; the size includes the ADD-S minima
 * (n_poses * ceil(n_points / 1024) * n_points doubles, about 25 MB at 20000 points and 8 poses) whether or not `syn` is given.
 * In the ADD-S sweep a NaN distance (a non-finite pose) is skipped, where numpy's min would propagate it. */
size_t opp_pose_metrics_workspace_bytes(int n_poses, int n_points);
int opp_pose_metrics(const float* model_pts, int n_points, const double* pose_pred, const double* pose_gt, const double* K,
                     const unsigned char* syn, const unsigned char* valid, int n_poses, double t_to_cm, double* out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- parameter update of the training step ---------------------------------
 * PyTorch's Adam / AdamW (optimizers/optimizers.py:4-13) behind its clip_grad_norm_ (Lightning's
 * `gradient_clip_val: 0.5`, train.yaml:32) over a LIST of fp32 tensors: one launch for the global gradient norm, one for
 * the update.  Both walk two DEVICE tables: one opp_optim_tensor per tensor and one opp_optim_chunk per workgroup; a chunk
 * is at most OPP_OPTIM_CHUNK elements of one tensor.  No atomics: the same inputs give the same bits. */
#define OPP_OPTIM_CHUNK 8192
typedef struct opp_optim_tensor {
  float* p;                /* parameter, n floats */
  const float* g;          /* its gradient (read only) */
  float* m;                /* first moment (exp_avg) */
  float* v;                /* second moment (exp_avg_sq) */
  long long n;
} opp_optim_tensor;
typedef struct opp_optim_chunk {
  int tensor;              /* index into the tensor table */
  int len;                 /* 1..OPP_OPTIM_CHUNK elements */
  long long start;         /* first element, a multiple of OPP_OPTIM_CHUNK */
} opp_optim_chunk;
/* The chunk length the library was built with (OPP_OPTIM_CHUNK). */
int opp_optim_chunk_elems(void);
/* The chunk table of a list of tensors -- a pure host function of the element counts numel [n_tensors], callable without a
 * device: tensor t gets ceil(numel[t] / OPP_OPTIM_CHUNK) consecutive chunks in tensor order (an empty tensor none), no chunk
 * spans two tensors.  *n_chunks receives their number; chunks (HOST array of max_chunks entries) may be NULL for the count
 * alone.  The caller copies the table to the device. */
int opp_optim_plan(const long long* numel, int n_tensors, opp_optim_chunk* chunks, long long max_chunks, long long* n_chunks);
/* partials[c] = grad_scale^2 x (sum of the squares of chunk c's gradient elements), accumulated in double: one slot per
 * workgroup, n_chunks doubles on the device.  Replaces the foreach norm + stack + norm of clip_grad_norm_. */
int opp_grad_sqnorm(const opp_optim_tensor* tensors, const opp_optim_chunk* chunks, int n_chunks, double grad_scale,
                    double* partials, void* stream);
/* One Adam (decoupled = 0: g' += wd p) or AdamW (decoupled != 0: p *= 1 - lr wd) step of the chunks [0, n_chunks) of
 * `chunks`, per element in fp32 in the order of operations of PyTorch's single-tensor Adam:
 *   g' = g grad_scale coef;  m += (g' - m)(1 - beta1);  v = v beta2 + (1 - beta2) g' g';
 *   p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),      bc1 = 1 - beta1^t, bc2 = 1 - beta2^t from the caller (host doubles).
 * g is not written.  n_partials > 0 clips: every workgroup sums partials [0, n_partials) (opp_grad_sqnorm over ALL tensors
 * of the step, whichever subset `chunks` covers) in index order, total_norm = sqrt(sum), coef = min(1, max_norm /
 * (total_norm + 1e-6)) as clip_grad_norm_ forms it, and workgroup 0 stores total_norm to norm_out (1 float, may be NULL);
 * a NaN norm propagates.  n_partials = 0: coef = 1, nothing is stored.  `chunks` may point into the middle of a table
 * (one launch per parameter group); chunk.tensor always indexes `tensors`. */
int opp_adam_step(const opp_optim_tensor* tensors, const opp_optim_chunk* chunks, int n_chunks, const double* partials,
                  int n_partials, double max_norm, float* norm_out, double grad_scale, double lr, double beta1, double beta2,
                  double eps, double weight_decay, int decoupled, double bc1, double bc2, void* stream);

/* Tuning aid (libraries built with -DOPP_TUNING only; otherwise returns an error): device buffer (4 x uint64 per
 * wave) for the phase time stamps written by the timed conv variants (tile_cfg 120 = 256x128 / 8 waves,
 * 121 = 128x128 / 4 waves, 122 = 128x128 / 8 waves); NULL disables. */
int opp_debug_timestamps(void* buf);

/* ---- live kernel timing for bench.py's roofline leg ---------------------------------------
 * Arms HIP-event timing (events recorded on the launch stream) of every launch of ONE kernel symbol:
 *   tile_cfg < 1000: a GEMM tile configuration (0 128x128/4 waves, 1 64x128, 2 64x64, 10/11 deeper prefetch,
 *                    20 256x128/8 waves, 22 128x256/8 waves, 24 128x192/8 waves, 25 128x128/8 waves, 26 64x128/8 waves,
 *                    27 128x224/8 waves on four fragment sets (bf16x3; outputs of <= 208 real / <= 224 stored columns), 30 64x256/8 waves + fused LayerNorm) of
 *                    kind 0 dense GEMM, 1 implicit-GEMM conv, 2 coarse score GEMM with fused softmax statistics;
 *   tile_cfg 1000 linear-attention KV gather, 1001 linear-attention apply, 1002 dual-softmax confidence pass,
 *            1003 the whole fine stage, 1004 fine-level attention (one workgroup per match), 1005 window gather,
 *            1006 fine head, 1007 / 1008 focal loss forward / backward (kind ignored).
 * opp_profile_stop synchronises and returns the summed time, the summed ALGORITHMIC work (FLOPs with unpadded
 * channel counts for GEMMs, bytes for the 1000+ symbols) and the number of launches measured. */
int opp_profile_start(int tile_cfg, int kind, int capacity_launches);
/* What the event pair itself adds to a short launch: an empty kernel timed exactly like an armed symbol (event before, event
 * after, all pairs enqueued back to back, one synchronisation at the end); *mean_us = mean elapsed time of `launches` pairs.
 * bench.py reports it beside the sub-15-us symbols and corrects their roofline fractions by it. */
int opp_profile_event_overhead(int launches, double* mean_us, void* stream);
/* The empty kernel's own duration: `launches` of them back to back between ONE event pair; *mean_us = elapsed / launches. */
int opp_profile_empty_kernel(int launches, double* mean_us, void* stream);
/* What an event pair adds to the reading of a real launch: a spin kernel of ~spin_us timed per launch between its own event pair (*pair_us)
 * and back to back between one pair (*b2b_us = its duration + the inter-kernel gap); pair_us - b2b_us is what bench.py subtracts. */
int opp_profile_event_calibration(int launches, double spin_us, double* pair_us, double* b2b_us, void* stream);
int opp_profile_stop(double* total_ms, double* total_work, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* OPP_HIP_H */
