/* vtgb.h -- C ABI of libvtgb.so: the MI355X (gfx950) kernels behind the VideoTGB
 * video -> LLM-prefix hot path.
 *
 * The reference (bigai-nlco/VideoTGB) is pure Python with no FFI of its own; each entry
 * point below replaces the torch op sequence of one reference function (cited as
 * file:line under /root/reference) and is what a ctypes stub on the reference side binds
 * (INTEGRATION.md).  Conventions, common to every call:
 *   - int return: 0 (VTGB_OK) or a negative VTGB_E* code; vtgb_last_error() returns a
 *     thread-local message for the last failing call on the calling thread;
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless the field
 *     comment says "host";  the library never allocates, frees or synchronises: the
 *     caller passes a workspace whose size comes from vtgb_<op>_workspace_bytes();
 *   - asynchronous on the given hipStream_t, re-entrant across streams, capturable
 *     into a hipGraph;
 *   - `dtype` selects the arithmetic of the GEMM/attention operands: VTGB_BF16 (bf16
 *     MFMA, fp32 accumulate, fp32 residual stream / LayerNorm / softmax) or VTGB_F32
 *     (fp32 everywhere: the exactness mode).  GEMM weights are passed in that dtype in
 *     the reference's nn.Linear layout [out_features, in_features] row-major; for
 *     VTGB_F32 these are the state_dict tensors themselves, for VTGB_BF16 a one-time
 *     vtgb_pack_bf16() of them.  Biases, LayerNorm parameters, embeddings: always fp32.
 *
 * Added at version 601 without a version bump (the existing entries are unchanged): vtgb_tgb_trunk / vtgb_tgb_resume and their
 * vtgb_tgb_split_args, the TGB split into a per-clip trunk and a per-question resume (see the TGB block below).
 */
#ifndef VTGB_H
#define VTGB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* vtgb_stream_t; /* == hipStream_t */

#define VTGB_VERSION 601 /* 601: vtgb_pair_conv_ex; vtgb_raft_encoder at VTGB_F16C8: every stride-1 3x3 of the residual blocks on f16c8 operands (weights[40] = int32 [12]); vtgb_raft_update at VTGB_F16C8: convf2 on f16c8 operands (weights[30] = int32 [10]), [20] = FlowHead.conv2 as the fp32 tail of conv1.  600: VTGB_F16C8 (vtgb_raft_update: the update block over fp16 + fp8-correction operands, weights[30] = scale bytes).  500: VTGB_BF16X3 (RAFT at fp32 accuracy on the bf16 MFMA), deterministic InstanceNorm moments, vtgb_gemm_skinny defer_reduce +
                            vtgb_llm_rmsnorm_parts / vtgb_llm_rope_cache_parts.  401: vtgb_gemm_train / vtgb_col_sum_f32 / vtgb_layernorm_train_* / vtgb_gelu_* (the training graph without operand copies or torch
                            elementwise passes); 400 = round 4: vtgb_llm_attention_rows / vtgb_llm_gated_act (the T5 language model of the BLIP-2 flavours on own kernels:
                            eval/utils/model.py:427-437), vtgb_llm_rope_cache with NULL tables = plain cache append; 300 = round 3: stem weight hi|lo layout; vtgb_attention_args.causal; vtgb_gemm_skinny without workspace when unsplit;
                            vtgb_llm_rope_cache_prefill; vtgb_attn_train_forward / backward; vtgb_comm_* / vtgb_allreduce_f32 */

#define VTGB_OK 0
#define VTGB_EINVAL (-1)       /* bad argument (NULL pointer, unsupported size, bad mode) */
#define VTGB_EWORKSPACE (-2)   /* workspace missing or too small                         */
#define VTGB_EHIP (-3)         /* a HIP launch failed                                    */
#define VTGB_EUNSUPPORTED (-4) /* shape outside what the kernels are built for           */

#define VTGB_F32 0
#define VTGB_BF16 1
#define VTGB_BF16X3 2 /* RAFT entry points only: split-bf16 operands (hi | lo pairs, three bf16 MFMA products per fp32 product) */
#define VTGB_F16C8 3  /* vtgb_raft_update / vtgb_raft_encoder only: fp16 main product + two OCP-fp8 correction products (fp32 accuracy class at 2/3 of VTGB_BF16X3's matrix work) */

int vtgb_version(void);
const char* vtgb_last_error(void);

/* One-time weight packing: dst[rows, cols_pad] bf16 <- src[rows, cols] fp32 (zero pad). */
int vtgb_pack_bf16(const float* src, void* dst, int64_t rows, int64_t cols, int64_t cols_pad,
                   vtgb_stream_t stream);

/* ---- K16: Gumbel top-k span selection -----------------------------------------------
 * Replaces eval/utils/model.py:101-113 (LSTP.generate), :315-327 (LSTP_blip2.generate),
 * src/models/LSTP_module.py:403-418.  idx[d][r] = first argmax over L of
 * (logit[r] + noise[d][r]) / tau, rows r < B from logits[..., 0] (start), rows >= B from
 * logits[..., 1] (end).  The caller supplies the Gumbel noise. */
typedef struct {
    const float* logits; /* [B, L, 2]      */
    const float* noise;  /* [draws, 2B, L] */
    int64_t* idx;        /* [draws, 2B]    */
    int32_t B, L, draws;
    float tau;
} vtgb_span_select_args;
int vtgb_span_select(const vtgb_span_select_args* a, vtgb_stream_t stream);

/* ---- K17: span -> candidate-frame index map + subsample -----------------------------
 * Replaces eval/utils/model.py:124-150 (variant A, :135) and :337-366 (variant B, :350);
 * src/models/LSTP_module.py:423-447, src/models/LSTP_SF_module.py:508-533.
 * Rounding rules: SURVEY.md Appendix B.  On an empty union -> range(N); duplicate-double
 * while shorter than nframe; float64 linspace midpoint subsample. */
#define VTGB_MAP_A 0 /* int(s / V * N)             (float32 divide, float32 multiply) */
#define VTGB_MAP_B 1 /* int(s * (N-1) / (V-1))     (int64 multiply, float32 divide)   */
typedef struct {
    const int64_t* sel;   /* [draws, 2B] from vtgb_span_select                        */
    const int32_t* V;     /* [B] per-clip video length, or NULL -> V_all              */
    int64_t* frame_idx;   /* [B, nframe]                                              */
    int32_t B, draws, V_all, N, nframe, variant;
} vtgb_span_to_frames_args;
int vtgb_span_to_frames(const vtgb_span_to_frames_args* a, vtgb_stream_t stream);

/* ---- K18: frame gather ---------------------------------------------------------------
 * Replaces eval/utils/model.py:122,151: out[b, i] = pixel_values[b, frame_idx[b, i]],
 * fp32, every output element written (the reference's zero-init buffer is fully
 * overwritten). frame_elems = C*H*W, must be a multiple of 4. */
typedef struct {
    const float* pixel_values; /* [B, N, frame_elems]      */
    const int64_t* frame_idx;  /* [B, nframe]              */
    float* out;                /* [B, nframe, frame_elems] */
    int32_t B, N, nframe;
    int64_t frame_elems;
} vtgb_gather_frames_args;
int vtgb_gather_frames(const vtgb_gather_frames_args* a, vtgb_stream_t stream);

/* ---- f3: frame preprocessing on the device ----------------------------------------------
 * Replaces the transform chain of get_frames (eval/utils/builder_utils.py:117-128: ResizeVideo ->
 * ToUint8 -> ToTHWC -> ToTensorVideo -> NormalizeVideo, i.e. src/gadgets/functional_video.py:33-41
 * resize (F.interpolate bilinear, align_corners=False, no antialias), truncation to uint8, /255
 * (:76-90) and (x - mean) / std (:93-110)) for decoded frames that are already in HBM.
 * frame_idx (optional): the 32-frame pick of builder_utils.py:133-141 applied on the fly -- output frame i is
 * source frame frame_idx[i]; NULL = identity (the flow_frames tensor). */
typedef struct {
    const uint8_t* raw;        /* [T, H0, W0, 3] decoded RGB frames                          */
    const int64_t* frame_idx;  /* [n_out] or NULL                                            */
    float* out;                /* [n_out, 3, size, size] fp32                                */
    int32_t T, H0, W0, n_out, size;
    float mean[3], std[3];
} vtgb_preprocess_args;
int vtgb_preprocess_frames(const vtgb_preprocess_args* a, vtgb_stream_t stream);

/* ---- a14: loss side of the LoRA training step (config C5) --------------------------------
 * vtgb_concat_text_io replaces LSTPModule.concat_text_input_output and the label construction around it
 * (src/models/LSTP_Vicuna_IVT_module.py:692-718 and :284-291): per row n = sum(input_atts),
 * llm = [input[:n] | output[1:] | input[n:]] (ids and attention mask), labels = -100 for the prefix_len visual
 * positions, for the first n text positions and for pad tokens, else the token id. */
typedef struct {
    const int64_t* input_ids;    /* [B, Li]  question tokens (right-padded)                  */
    const int64_t* input_atts;   /* [B, Li]                                                  */
    const int64_t* output_ids;   /* [B, Lo]  answer tokens (first one, BOS, is dropped)      */
    const int64_t* output_atts;  /* [B, Lo]                                                  */
    int64_t* llm_ids;            /* [B, Li + Lo - 1]                                         */
    int64_t* llm_atts;           /* [B, Li + Lo - 1]                                         */
    int64_t* input_len;          /* [B] or NULL: the n of each row (input_part_targets_len)  */
    int64_t* labels;             /* [B, prefix_len + Li + Lo - 1] or NULL                    */
    int64_t pad_id;
    int32_t B, Li, Lo, prefix_len;
} vtgb_concat_text_io_args;
int vtgb_concat_text_io(const vtgb_concat_text_io_args* a, vtgb_stream_t stream);

/* Shifted cross-entropy (LSTP_Vicuna_IVT_module.py:297-299, :325-326: logits[..., :-1, :] against labels[..., 1:],
 * CrossEntropyLoss(reduction="mean"), ignore_index -100) without the shifted copies: forward reads the logits once
 * (rows whose target is ignored are skipped), backward writes d loss / d logits for all S positions. */
typedef struct {
    int32_t dtype, B, S, V;      /* logits dtype VTGB_F32 / VTGB_BF16                        */
    const void* logits;          /* [B, S, V]                                                */
    const int64_t* labels;       /* [B, S]                                                   */
    float* lse;                  /* [B, S-1] log-sum-exp per scored row (kept for backward)  */
    float* row_loss;             /* [B, S-1] scratch                                         */
    float* loss;                 /* [2]: mean loss, number of scored rows                    */
    const float* grad_out;       /* [1] upstream gradient (backward)                         */
    void* dlogits;               /* [B, S, V] same dtype as logits (backward)                */
} vtgb_shifted_ce_args;
int vtgb_shifted_ce_forward(const vtgb_shifted_ce_args* a, vtgb_stream_t stream);
int vtgb_shifted_ce_backward(const vtgb_shifted_ce_args* a, vtgb_stream_t stream);

/* ---- K1-K6: EVA-ViT-g vision tower ----------------------------------------------------
 * Replaces InstructBlipVisionModel.forward, src/models/components/xinstructblip.py:515-558
 * (embeddings :113-122, 39 x encoder layer :233-269 with attention :162-204 and MLP
 * :216-220, post_layernorm :545) and the identical Blip2VisionModel (xblip2.py:500).
 * weights (host array of device pointers), in this order:
 *   [0] patch_embedding.weight  `dtype` [hidden, kpad]   (kpad: see vtgb_vit_patch_kpad)
 *   [1] patch_embedding.bias  [2] class_embedding  [3] position_embedding [tokens, hidden]
 *   [4] post_layernorm.weight [5] post_layernorm.bias
 *   then per layer l, at 6 + 18*l:
 *   +0 layer_norm1.weight +1 layer_norm1.bias +2 self_attn.qkv.weight `dtype` [3h, h]
 *   +3 self_attn.qkv.bias +4 self_attn.projection.weight `dtype` +5 .bias
 *   +6 layer_norm2.weight +7 layer_norm2.bias +8 mlp.fc1.weight `dtype` +9 .bias
 *   +10 mlp.fc2.weight `dtype` +11 .bias
 *   +12 .. +17 optional, VTGB_BF16 only (all six of EVERY layer or none -- a partially filled block is VTGB_EINVAL since version 600; none = the
 *   LayerNorms run as their own passes; with them present +2 and +8 are not read and may be NULL): the two LayerNorms FOLDED into the
 *   GEMMs that follow them -- LN(x) W^T + b = rstd (x W'^T - mean cs) + c with
 *   +12 W'_qkv = bf16(qkv.weight * layer_norm1.weight[None, :]) [3h, h]   +13 cs = row sums of W'_qkv (of the bf16 values), fp32 [3h]
 *   +14 c = qkv.weight @ layer_norm1.bias + qkv.bias, fp32 [3h]           +15 / +16 / +17 the same for mlp.fc1 with layer_norm2 [mlp]:
 *   the producer of the residual stream (projection / fc2 epilogue) then also writes bf16(x) and the rows' moments, and no stand-alone
 *   LayerNorm pass is left between the GEMMs of a layer (version 500) */
#define VTGB_VIT_NW_GLOBAL 6
#define VTGB_VIT_NW_LAYER 18
typedef struct {
    int32_t dtype, n_frames, image, patch, hidden, heads, mlp, layers;
    float eps;
    const float* pixel_values;  /* [n_frames, 3, image, image] fp32                    */
    const void* const* weights; /* host array                                          */
    float* out_f32;             /* [n_frames, tokens, hidden] fp32 or NULL             */
    void* out_act;              /* same, in `dtype`, or NULL (feeds vtgb_qformer)      */
    void* workspace;
    size_t workspace_bytes;
} vtgb_vit_args;
int32_t vtgb_vit_patch_kpad(int32_t dtype, int32_t patch);
size_t vtgb_vit_workspace_bytes(const vtgb_vit_args* a);
int vtgb_vit_forward(const vtgb_vit_args* a, vtgb_stream_t stream);

/* ---- K7-K10: Q-Former -----------------------------------------------------------------
 * Replaces InstructBlipQFormerModel.forward xinstructblip.py:1122-1242 (has_text = 1:
 * embeddings :1018-1046, layers :814-883, attention :611-694) and Blip2QFormerModel.forward
 * xblip2.py:1063-1174 (has_text = 0: layernorm(query_embeds) :1108).  Output: the query
 * rows [:, :n_query] of the last layer.
 * weights: has_text: [0] embeddings.word_embeddings.weight [1] embeddings.position_embeddings.weight
 *                    [2] embeddings.layernorm.weight [3] .bias
 *          else:     [0] NULL [1] NULL [2] layernorm.weight [3] layernorm.bias
 *   then per layer l at 4 + 32*l (entries of absent sub-blocks are NULL):
 *   +0..+5  attention.attention.{query,key,value}.{weight `dtype`, bias}
 *   +6 attention.output.dense.weight `dtype` +7 .bias +8 attention.output.LayerNorm.weight +9 .bias
 *   +10..+15 crossattention.attention.{query,key,value}.{weight,bias}  (key/value: [h, enc_hidden])
 *   +16 crossattention.output.dense.weight +17 .bias +18 crossattention.output.LayerNorm.weight +19 .bias
 *   +20 intermediate_query.dense.weight +21 .bias +22 output_query.dense.weight +23 .bias
 *   +24 output_query.LayerNorm.weight +25 .bias
 *   +26 intermediate.dense.weight +27 .bias +28 output.dense.weight +29 .bias
 *   +30 output.LayerNorm.weight +31 .bias                                              */
#define VTGB_QF_NW_GLOBAL 4
#define VTGB_QF_NW_LAYER 32
typedef struct {
    int32_t dtype, n_frames, n_query, n_text, hidden, heads, ffn, layers, cross_freq;
    int32_t enc_tokens, enc_hidden, has_text;
    float eps;
    const void* image_embeds;   /* [n_frames, enc_tokens, enc_hidden] in `dtype`        */
    const float* query_tokens;  /* [n_query, hidden] fp32                               */
    const int64_t* text_ids;    /* [n_frames, n_text] or NULL                           */
    const int64_t* text_mask;   /* [n_frames, n_text] (1 = attend) or NULL = all ones   */
    const int64_t* image_mask;  /* [n_frames, enc_tokens] or NULL = all ones            */
    const void* const* weights; /* host array                                           */
    float* out_f32;             /* [n_frames, n_query, hidden]                          */
    void* workspace;
    size_t workspace_bytes;
} vtgb_qformer_args;
size_t vtgb_qformer_workspace_bytes(const vtgb_qformer_args* a);
int vtgb_qformer_forward(const vtgb_qformer_args* a, vtgb_stream_t stream);

/* ---- K11: frame pooling + language_projection -----------------------------------------
 * mean: eval/utils/model.py:186-195 and the ragged `widths` form of
 * src/models/LSTP_Vicuna_IVT_module.py:244-249 (width 0 -> zero row, i.e. bias only);
 * concat: src/models/LSTP_module.py:477-481.
 * out: mean [n_clips, n_query, out_dim]; concat [sum(widths) * n_query, out_dim].      */
#define VTGB_POOL_MEAN 0
#define VTGB_POOL_CONCAT 1
typedef struct {
    int32_t dtype, n_clips, n_query, hidden, out_dim, mode;
    const float* query_out;  /* [sum(widths), n_query, hidden] fp32 */
    const int32_t* widths;   /* host array [n_clips]                */
    const void* proj_w;      /* `dtype` [out_dim, hidden]           */
    const float* proj_b;     /* [out_dim]                           */
    float* out;
    void* workspace;
    size_t workspace_bytes;
} vtgb_pool_project_args;
size_t vtgb_pool_project_workspace_bytes(const vtgb_pool_project_args* a);
int vtgb_pool_project(const vtgb_pool_project_args* a, vtgb_stream_t stream);

/* ---- K12-K15: Temporal Grounding Bridge encoder ---------------------------------------
 * Replaces RopeBertModel.forward src/models/components/xropebert.py:1048-1169 called with
 * encoder_embeds=of (TemporalOFEmbedding :103-129, RopeBertEmbeddings :190-208, rotary
 * attention :243-377, layers :450-533, mode switch :621-634, mrc_head :1164).
 * weights: [0] embeddings.word_embeddings.weight [1] embeddings.token_type_embeddings.weight
 *   [2] embeddings.LayerNorm.weight [3] .bias [4] temporal_embeddings.bos [5] .eos
 *   [6] temporal_embeddings.projection.weight fp32 [hidden, 2*patch*patch] [7] .bias
 *   [8] temporal_embeddings.fc.weight [9] .fc.bias [10] temporal_embeddings.frame_pos_embed.weight
 *   [11] temporal_embeddings.ln.weight [12] .ln.bias [13] encoder.embed_positions.weight
 *   [14] encoder.c_embed_positions.weight [15] mrc_head.weight fp32 [2, hidden] [16] mrc_head.bias
 *   then per layer l at 17 + 26*l (crossattention entries NULL below fusion_layer):
 *   +0..+5 attention.self.{query,key,value}.{weight `dtype`, bias}
 *   +6 attention.output.dense.weight `dtype` +7 .bias +8 attention.output.LayerNorm.weight +9 .bias
 *   +10..+15 crossattention.self.{query,key,value}.{weight,bias}
 *   +16 crossattention.output.dense.weight +17 .bias +18 crossattention.output.LayerNorm.weight +19 .bias
 *   +20 intermediate.dense.weight +21 .bias +22 output.dense.weight +23 .bias
 *   +24 output.LayerNorm.weight +25 .bias                                              */
#define VTGB_TGB_NW_GLOBAL 17
#define VTGB_TGB_NW_LAYER 26
#define VTGB_TGB_MODE_TEXT 0       /* layers [0, fusion_layer)  ("text" / "vision") */
#define VTGB_TGB_MODE_FUSION 1     /* layers [fusion_layer, layers)                 */
#define VTGB_TGB_MODE_MULTIMODAL 2 /* all layers                                    */
typedef struct {
    int32_t dtype, B, L, n_text, hidden, heads, ffn, layers, fusion_layer, mode, image, patch;
    float eps;
    const float* of;            /* [B, L, 2, image, image] fp32 */
    const int64_t* of_mask;     /* [B, L+2]                     */
    const int64_t* text_ids;    /* [B, n_text]                  */
    const int64_t* text_mask;   /* [B, n_text]                  */
    const void* const* weights; /* host array                   */
    float* seq_out;             /* [B, L+2, hidden] or NULL     */
    float* logits;              /* [B, L, 2]                    */
    void* workspace;
    size_t workspace_bytes;
} vtgb_tgb_args;
size_t vtgb_tgb_workspace_bytes(const vtgb_tgb_args* a);
int vtgb_tgb_forward(const vtgb_tgb_args* a, vtgb_stream_t stream);

/* ---- the same encoder split at its first question-dependent layer (clip sessions: many questions, one clip) -----------------
 * vtgb_tgb_trunk runs the question-independent part on ONE clip (B == 1): TemporalOFEmbedding + its LayerNorm (xropebert.py:103-129)
 * and the layers of `mode` before the first cross-attention layer -- [0, fusion_layer) for multi_modal, none for fusion, all for
 * text / vision (:621-634) -- and leaves the residual stream in trunk (fp32) AND trunk_act (`dtype`, what the next layer's GEMMs
 * read).  vtgb_tgb_resume runs B question rows against one trunk: the trunk replicated into B row blocks, RopeBertEmbeddings on
 * the question (:190-208), the self / cross masks, the remaining layers and mrc_head (:1164).  Both share vtgb_tgb_forward's
 * launch sequences and descriptors, so trunk + resume equals vtgb_tgb_forward on the clip repeated B times BIT FOR BIT (both
 * dtypes, every mode, padded text masks).  Same weights table as vtgb_tgb_args; the *_workspace_bytes queries need no GPU and
 * return 0 on bad arguments (last error set: "INVALID MODE", "bad dims"). */
typedef struct {
    int32_t dtype, B, L, n_text, hidden, heads, ffn, layers, fusion_layer, mode, image, patch;  /* trunk: B == 1, n_text unused */
    float eps;
    const float* of;            /* trunk: [1, L, 2, image, image] fp32 (resume: unused)        */
    const int64_t* of_mask;     /* [1, L+2], the clip's (both)                                 */
    const int64_t* text_ids;    /* resume: [B, n_text]                                         */
    const int64_t* text_mask;   /* resume: [B, n_text]                                         */
    const void* const* weights; /* host array, as vtgb_tgb_args                                */
    float* trunk;               /* [L+2, hidden] fp32: written by the trunk, read by resume    */
    void* trunk_act;            /* [L+2, hidden] `dtype`: same                                 */
    float* seq_out;             /* resume: [B, L+2, hidden] or NULL                            */
    float* logits;              /* resume: [B, L, 2]                                           */
    void* workspace;
    size_t workspace_bytes;
} vtgb_tgb_split_args;
size_t vtgb_tgb_trunk_workspace_bytes(const vtgb_tgb_split_args* a);
int vtgb_tgb_trunk(const vtgb_tgb_split_args* a, vtgb_stream_t stream);
size_t vtgb_tgb_resume_workspace_bytes(const vtgb_tgb_split_args* a);
int vtgb_tgb_resume(const vtgb_tgb_split_args* a, vtgb_stream_t stream);

/* ---- building blocks, exported for the per-kernel parity tests and the roofline bench ----
 * out[M, N] = epilogue(A[M, K] . W[N, K]^T + bias).  A, W in `dtype`; K % 8 == 0.       */
#define VTGB_EPI_STORE 0      /* out `dtype`  = acc + bias                      */
#define VTGB_EPI_GELU 1       /* out `dtype`  = gelu_erf(acc + bias)            */
#define VTGB_EPI_RESID_F32 2  /* out fp32     = acc + bias + resid (may alias)  */
#define VTGB_EPI_STORE_F32 3  /* out fp32     = acc + bias                      */
typedef struct {
    int32_t dtype, M, N, K, epilogue;
    const void* A;
    int64_t lda;
    const void* W;
    int64_t ldw;
    const float* bias;  /* [N] or NULL */
    const float* resid; /* [M, ldo] fp32 (VTGB_EPI_RESID_F32) */
    void* out;
    int64_t ldo;
} vtgb_gemm_args;
int vtgb_gemm(const vtgb_gemm_args* a, vtgb_stream_t stream);

/* softmax(scale * Q K^T + key_mask) V over [batch, heads]; Q/K/V/out token-major in `dtype`. */
typedef struct {
    int32_t dtype, batch, heads, head_dim, s_q, s_kv;
    const void* q;
    const void* k;
    const void* v;
    int64_t q_tok_stride, kv_tok_stride; /* elements between consecutive tokens        */
    int64_t q_batch_stride, kv_batch_stride;
    const float* key_mask;               /* additive [batch, s_kv] fp32 or NULL        */
    const float* rope_q;                 /* [>= s_q, head_dim] sin|cos table or NULL   */
    const float* rope_k;                 /* [>= s_kv, head_dim] or NULL                */
    float scale;
    void* out;                           /* [batch, s_q, heads*head_dim] in `dtype`    */
    int64_t out_tok_stride, out_batch_stride;
    int32_t causal;                      /* != 0: query q attends keys <= q + (s_kv - s_q) (the LLM's prefill) */
} vtgb_attention_args;
int vtgb_attention(const vtgb_attention_args* a, vtgb_stream_t stream);

/* Tiled attention for the language model's prefill (HF LlamaAttention as called from eval/utils/model.py:217; added at version 601
 * without a version bump): bf16 in / out, fp32 scores and accumulator, online softmax over 64-key tiles, so s_kv is not bound by
 * LDS (<= 4096), and grouped-query heads: query head h reads K/V head h / (heads / kv_heads) in place.  head_dim 64 or 128.
 * Q is [batch, s_q, heads * head_dim], K/V are [batch, s_kv, kv_heads * head_dim], token-major with the strides below.
 * key_mask: a value <= finfo(float32).min masks the key HARD -- weight exactly 0 and its K/V rows are never read (a pad slot may hold
 * NaN); any other value is added to the scaled score.  A query with no visible key gets an all-zero output row.  A row's result does
 * not depend on batch, on the other rows or on run order (no atomics, keys are not split over workgroups).
 * Errors, on the host before any launch: VTGB_EINVAL for a NULL args / q / k / v / out, a non-positive size or heads % kv_heads != 0;
 * VTGB_EUNSUPPORTED for head_dim outside {64, 128}, s_kv > 4096, batch or heads > 65535, strides that break 16-byte alignment
 * (token and batch strides of q / k / v multiples of 8 elements, of out multiples of 4), or base pointers that do: q / k / v 16-byte,
 * out 8-byte, key_mask 4-byte aligned (the kernel moves 16-byte pieces of Q, K and V and 8-byte pieces of the output). */
typedef struct {
    int32_t batch, heads, kv_heads, head_dim, s_q, s_kv;
    const void* q;
    const void* k;
    const void* v;
    int64_t q_tok_stride, kv_tok_stride; /* elements between consecutive tokens                         */
    int64_t q_batch_stride, kv_batch_stride;
    const float* key_mask;               /* [batch, s_kv] fp32 (see above) or NULL                      */
    float scale;
    int32_t causal;                      /* != 0: query q attends keys <= q + (s_kv - s_q)              */
    void* out;                           /* [batch, s_q, heads*head_dim] bf16                           */
    int64_t out_tok_stride, out_batch_stride;
} vtgb_attention_tiled_args;
int vtgb_attention_tiled(const vtgb_attention_tiled_args* a, vtgb_stream_t stream);

/* Causal attention of a chunk of queries over the language model's KV cache: the chunked prefill of prompts past the one-shot prefill's
 * bound (added at version 601 without a version bump).  q [batch, s_q, heads * head_dim] bf16 (token and batch strides below) are the
 * prompt positions q0 .. q0 + s_q - 1; kc / vc [batch, kv_heads, tmax, head_dim] are the decoder's caches, contiguous: bf16 (ks = vs =
 * NULL), or uint8 e4m3 codes with ks / vs [batch, kv_heads, tmax] fp32 power-of-two row scales (vtgb_llm_decode_attention_split_fp8's
 * layout; value = code * scale, exactly a bf16 number).  Query i sees cache rows 0 .. q0 + i; nothing at or past row q0 + s_q is read.
 * key_valid [batch, tmax] uint8 or NULL (the decode kernels' convention): a key with 0 gets weight exactly 0 and neither its K / V row nor
 * its codes or scales are read (a pad slot may hold NaN).  A query with no visible key gets an all-zero output row.  out [batch, s_q,
 * heads * head_dim] bf16.  Query head h reads K/V head h / (heads / kv_heads) in place.
 * The tile partition and the per-tile arithmetic are vtgb_attention_tiled's, so the output equals vtgb_attention_tiled's with
 * s_kv = q0 + s_q, causal, on the same K / V values laid out token-major (key_valid 0 <-> a hard key_mask), bit for bit, wherever that
 * entry takes the call; an fp8 cache gives the bits of the bf16 cache of its dequantised values.  A row's result does not depend on
 * batch, on tmax, on the other rows or on run order.
 * Limits: head_dim 64 or 128, heads % kv_heads == 0, q0 >= 0, s_q > 0, q0 + s_q <= tmax <= 16384.
 * Errors, on the host before any launch: VTGB_EINVAL for a NULL args / q / kc / vc / out, a non-positive size, a negative q0,
 * heads % kv_heads != 0, or exactly one of ks / vs; VTGB_EUNSUPPORTED for head_dim outside {64, 128}, tmax > 16384, q0 + s_q > tmax,
 * batch or heads > 65535, strides that break 16-byte alignment (q multiples of 8 elements, out of 4), or base pointers that do:
 * q / kc / vc 16-byte, out 8-byte, ks / vs 4-byte aligned. */
typedef struct {
    int32_t batch, heads, kv_heads, head_dim, s_q;
    int32_t q0;                            /* cache row of the chunk's first query                        */
    int32_t tmax;                          /* slots per (batch, K/V head) of the caches                   */
    float scale;
    const void* q;
    const void* kc;                        /* bf16, or e4m3 codes when ks / vs are given                  */
    const void* vc;
    const float* ks;                       /* [batch, kv_heads, tmax] fp32 row scales, or NULL (bf16)     */
    const float* vs;
    const uint8_t* key_valid;              /* [batch, tmax] or NULL                                       */
    int64_t q_tok_stride, q_batch_stride;  /* elements                                                    */
    void* out;                             /* [batch, s_q, heads*head_dim] bf16                           */
    int64_t out_tok_stride, out_batch_stride;
} vtgb_attention_cached_args;
int vtgb_attention_cached(const vtgb_attention_cached_args* a, vtgb_stream_t stream);

/* LayerNorm over the last dim of fp32 rows; writes fp32 and/or `dtype` copies. */
typedef struct {
    int32_t dtype, M, D;
    float eps;
    const float* x;
    const float* gamma;
    const float* beta;
    float* out_f32; /* or NULL */
    void* out_act;  /* or NULL */
} vtgb_layernorm_args;
int vtgb_layernorm(const vtgb_layernorm_args* a, vtgb_stream_t stream);

/* ---- a2 / f1: RAFT (src/models/components/xraft.py:102-156) --------------------------------------
 * Three entry points cover RAFT.forward: vtgb_raft_encoder (fnet / cnet), vtgb_raft_corr (CorrBlock.__init__) and
 * vtgb_raft_update (the refinement loop, mask head and convex upsample).  `dtype` selects the arithmetic of all
 * three: VTGB_BF16 = bf16 MFMA implicit-GEMM convolutions over NHWC bf16 activations, fp32 accumulation, fp32
 * hidden state / flow / norms, IEEE-half correlation pyramid (a reduced-precision mode the reference does not have);
 * VTGB_F32 = fp32 operands and FMAs everywhere, k summed in order -- the exactness mode, which is how the reference
 * runs RAFT (xraft.py:118-119; since version 500 on the fp32-input matrix instruction, the same fmaf chain bit for bit; the convolutions sum k in
 * four interleaved in-order chains, added in a fixed order: a quarter of one chain's rounding error, csrc/conv_f32.hip).
 * VTGB_BF16X3 (version 500) = the reference's fp32 ACCURACY on the bf16 matrix cores: every convolution operand is a bf16 pair
 * (hi = bf16(x), lo = bf16(x - hi): 16 significant bits), x . w ~ hi . Wh + lo . Wh + hi . Wl with fp32 accumulation; activations
 * are stored as rows [hi(C) | lo(C)], gates / flow / correlation pyramid / lookup stay fp32 (the pyramid from split-bf16 products).
 * Flows within 1e-4 relative RMS of the reference's under input-sensitive weights (tests/test_gpu_raft.py), 3 x the MFMA work of VTGB_BF16.
 * Weight tables at VTGB_BF16X3: every MFMA convolution [C_out, taps, 3 C_in] in the K order below with the channel blocks
 * [Wh | Wh | Wl] per source of the (virtual) input concatenation (bf16; built by ops.split3); vtgb_raft_update: [4] convf1 as at VTGB_F32,
 * [10] .. [17] the GRU convolutions over [h(128) | motion(126) | flow(2)] and [26] .. [29] their `inp` parts (always present: the loop-invariant
 * third is computed once per call into fp32 start maps), [24] / [25] mask.2 with its 0.25 folded in; vtgb_raft_encoder: [0] the stem
 * [64, 4 (tY), 3 x 64] scaled by 2/255, the 1x1 head [256, 3 x 128].
 * VTGB_F16C8 (version 600; vtgb_raft_update and vtgb_raft_encoder -- the correlation volume of that mode runs at VTGB_BF16X3; vtgb_raft_encoder at
 * VTGB_F16C8 is the VTGB_BF16X3 encoder with the ten stride-1 3x3 convolutions of its residual blocks [both convolutions of layer1.0, layer1.1,
 * layer2.1, layer3.1 and conv2 of layer2.0, layer3.0: entries 2, 4, 8, 10, 16, 20, 22, 28, 32, 34] on these operands and weights[40] = DEVICE
 * int32 [12], the scale byte of block b's conv1 / conv2 at [2 b] / [2 b + 1]; the stem, the stride-2 convolutions, the 1x1 downsamples and the 1x1
 * head stay split-bf16): the nine large
 * convolutions of the update block ([0] convc1, [2] convc2, [8] conv, [10] / [12] / [14] / [16] the GRU's, [18] flow_head.conv1, [22] mask.0) take
 * their operands as  x . w ~ xh . Wh  (fp16 x fp16)  +  2^-11/sw (xl' . Wh8 + xh8 . Wl')  (OCP fp8 on the block-scaled matrix instruction, twice the
 * fp16 rate), xh = fp16(x), xl' = e5m2((x - xh) 2^11), xh8 = e5m2(x), Wh = fp16(w), Wh8 = e4m3(w sw), Wl' = e4m3((w - Wh) sw 2^11), sw a power of two
 * per layer: the corrections are 2^-11 of the product, so 3-4 significant bits on each side leave ~2^-16 -- the bf16 pair's level (tests/
 * test_gpu_raft.py holds this mode to the bf16x3 mode's bounds).  Their weights are [C_out, K] 16-bit units with K = per source (fp16 [taps, C] |
 * correction bytes [taps, C / 4 groups of (Wh8 x 4, Wl' x 4)]), each half in the 64-channel-chunk-major K order below (ops.h8_conv_pack);
 * weights[30] = DEVICE int32 [10]: the E8M0 byte of 2^-11 / sw of those nine convolutions in the order above, then of [6] convf2 (3x3, 128 -> 64: an
 * f16c8 convolution as well, its input -- convf1's output -- an f16c8 pair).  Everything else in the table is as at VTGB_BF16X3.  Activations beyond +-57344 saturate (e5m2's range; RAFT's are normalised features, gates and correlations of unit-scale features).
 * Convolution weights are packed [C_out, K] in `dtype` with K running 64-channel chunk
 * major, tap minor, channel-in-chunk innermost (written [C_out, KH,KW,C_in] below for the shapes only).
 *
 * vtgb_raft_update replaces the refinement loop xraft.py:135-156: per iteration CorrBlock.__call__
 * (raft_utils/corr.py:29-50; the reference's optional `alt_cuda_corr`, corr.py:63-91, is the CUDA counterpart of the
 * lookup kernel), BasicUpdateBlock (raft_utils/update.py:123-144: BasicMotionEncoder :75-97, SepConvGRU :39-65,
 * FlowHead :6-18), then the mask head and upsample_flow (xraft.py:88-99) of the last iteration.  At VTGB_BF16 the lookup and
 * convc1 are one launch (the 324 taps of a pixel never leave the CU).  n_pairs * H8 * W8 < 2^28 coarse pixels per call.
 * weights (host array of device pointers):
 *   [0] encoder.convc1.weight [256, 384] (324 input channels zero-padded to 384) [1] .bias
 *   [2] encoder.convc2.weight [192, 3,3,256] [3] .bias
 *   [4] encoder.convf1.weight -- VTGB_BF16: bf16 [128, 56 taps, {x,y,x,y}] (49 taps zero-padded; the flow enters as a
 *       bf16 head + bf16 remainder); VTGB_F32: fp32 [98, 128] (k = c*49 + ky*7 + kx, output channel minor)   [5] .bias
 *   [6] encoder.convf2.weight [64, 3,3,128]  [7] .bias   [8] encoder.conv.weight [126, 3,3,256]     [9] .bias
 *   [10] gru.convz1|convr1.weight [256, 1,5,384] [11] bias [256]  [12] gru.convq1.weight [128, 1,5,384] [13] .bias
 *   [14] gru.convz2|convr2.weight [256, 5,1,384] [15] bias [256]  [16] gru.convq2.weight [128, 5,1,384] [17] .bias
 *   [18] flow_head.conv1.weight [256, 3,3,128] [19] .bias  [20] flow_head.conv2.weight [32, 256], row tap*2+o (18 rows zero-padded) [21] .bias
 *   [22] mask.0.weight [256, 3,3,128] [23] .bias           [24] mask.2.weight [576, 256] [25] .bias
 *   [26..29] optional, VTGB_BF16 only (all four or none; NULL = the plain form above): the `inp` split of the GRU
 *       convolutions.  `inp` (input channels 128..255) does not change over the refinement iterations, so its contribution
 *       is computed once per call and the 80 GRU launches contract over the other 256 channels only.  With the split,
 *       [10] / [12] / [14] / [16] hold the [h(128) | motion(126) | flow(2)] channels: [256 or 128, taps, 256], and
 *       [26] gru.convz1|convr1 inp part [256, 1,5,128]   [27] gru.convq1 inp part [128, 1,5,128]
 *       [28] gru.convz2|convr2 inp part [256, 5,1,128]   [29] gru.convq2 inp part [128, 5,1,128]
 * Biases fp32.  GRU input channels are [h(128) | inp(128) | motion(126) | flow(2)] as in the reference. */
#define VTGB_RAFT_NW 30
typedef struct {
    int32_t dtype, n_pairs, H8, W8, iters;
    const float* net;           /* [n_pairs, 128, H8, W8] tanh(cnet[:, :128])   (xraft.py:126-127) */
    const float* inp;           /* [n_pairs, 128, H8, W8] relu(cnet[:, 128:])                      */
    const void* corr[4];        /* pyramid level l: [n_pairs*H8*W8, H8>>l, W8>>l] (corr.py:19-27), fp32 or fp16 (corr_f16) */
    const void* const* weights; /* host array                                                      */
    float* flow_up;             /* [n_pairs, 2, 8*H8, 8*W8]                                        */
    void* workspace;
    size_t workspace_bytes;
    int32_t corr_f16;           /* 0: fp32 pyramid; 1: IEEE half (what vtgb_raft_corr writes in VTGB_BF16 mode)  */
    const float* cnet_nhwc;     /* optional: the context encoder's raw output [n_pairs*H8*W8, 256] (vtgb_raft_encoder layout);
                                   net = tanh(first 128), inp = relu(last 128) are then taken from it and net/inp may be NULL */
    const float* flow_init;     /* optional [n_pairs, 2, H8, W8]: coords1 = coords0 + flow_init (xraft.py:131-132)    */
} vtgb_raft_update_args;
size_t vtgb_raft_update_workspace_bytes(const vtgb_raft_update_args* a);
int vtgb_raft_update(const vtgb_raft_update_args* a, vtgb_stream_t stream);

/* Unit-level surface of the VTGB_F16C8 operand format (version 600; what tests/test_gpu_h8.py checks piece by piece -- vtgb_raft_update is built from
 * these): vtgb_pair_pack writes fp32 rows [M, C] (C % 4 == 0) as pair rows [M, 2 * ld_pair 16-bit units] -- fmt VTGB_F16C8: fp16 values at unit c, the
 * eight correction bytes of channels 4g .. 4g+3 at unit ld_pair + 4g (csrc/pair_h8.h); fmt VTGB_BF16X3: bf16 hi at unit c, bf16 lo at unit ld_pair + c.
 * Channels [C, ld_pair) are written as zeros.  vtgb_pair_conv: one stride-1 "same" convolution (RAFT update block, raft_utils/update.py:75-97) over
 * f16c8 pair rows: out = act(conv(x) + bias) as a pair row again (out_fmt VTGB_F16C8 or VTGB_BF16X3), x = C1 channels from `a` (+ C1 more from `a2`:
 * a virtual concatenation), weights / scale as vtgb_raft_update's table holds them (ops.h8_conv_pack; scale = device int32: the E8M0 byte). */
int vtgb_pair_pack(int32_t fmt, const float* x, void* out, int64_t M, int32_t C, int32_t ld_pair, vtgb_stream_t stream);
typedef struct {
    int32_t M, N, H, W, KH, KW, C1;   /* M = images * H * W output pixels; N output channels (even); C1 % 64 == 0 input channels per source */
    const void* a;                    /* pair rows [M, 2 * C1 units] */
    const void* a2;                   /* optional second source, same width */
    const void* weights;              /* [N, taps * 2 * C1 * sources] 16-bit units */
    const int32_t* scale;             /* device: E8M0 byte of 2^-11 / sw */
    const float* bias;                /* optional [N] */
    int32_t act;                      /* 0 none, 1 relu */
    int32_t out_fmt;                  /* VTGB_F16C8 or VTGB_BF16X3 */
    void* out;                        /* pair rows [M, 2 * ld_out units], second half at unit ld_out */
    int32_t ld_out;                   /* >= N, % 4 == 0 */
} vtgb_pair_conv_args;
int vtgb_pair_conv(const vtgb_pair_conv_args* a, vtgb_stream_t stream);
/* The same convolution with one of the three other epilogues the RAFT launches use (version 601; unit tests of those epilogues): exactly one of
 *   resid    -- the ResidualBlock tail (extractor.py:56-60): out = relu(resid + act(conv(x) + bias)) as a pair row; resid = f16c8 pair rows [M, 2 * ld_resid
 *               units]; N <= 128, N % 4 == 0 (cnet's blocks at VTGB_F16C8);
 *   tail_w   -- FlowHead (update.py:10-18): N == 256; tail_out [M, 32] fp32 = act(conv(x) + bias) . W2, the 18 per-tap products of the following 3x3
 *               convolution (columns 18 .. 31: zero weights), formed from the accumulators in exact fp32; tail_w = W2 [256, 32] fp32 in the epilogue's lane
 *               order (ops.flow_tail_pack); `out` is not written;
 *   out_f32  -- fp32 rows [M, ld_f32] instead of a pair (N <= 128, N % 4 == 0, act == 0: fnet's convolutions in front of an InstanceNorm)
 * may be non-NULL (all NULL: vtgb_pair_conv). */
typedef struct {
    vtgb_pair_conv_args conv;
    const void* resid;
    int32_t ld_resid;
    const float* tail_w;
    float* tail_out;
    float* out_f32;
    int32_t ld_f32;
} vtgb_pair_conv_ex_args;
int vtgb_pair_conv_ex(const vtgb_pair_conv_ex_args* a, vtgb_stream_t stream);

/* Unit-level surface of vtgb_raft_update's fused f16c8 launch "correlation lookup + convc1" (corr.py:29-50, update.py:88: cor = relu(convc1(corr)),
 * 1x1, 324 -> 256): for every pixel the 4 x 81 bilinear taps of the pyramid around (pixel + flow), as f16c8 operands (csrc/pair_h8.h) against the
 * table's convc1 weights (ops.h8_conv_pack of the [256, 1, 1, 384] zero-padded weight; scale = device int32: the E8M0 byte), + bias, ReLU -> c1 as
 * f16c8 pair rows.  variant 1: the split-K tile vtgb_raft_update launches (two workgroups per CU); variant 0: the whole-K tile it replaced (one
 * workgroup per CU) -- the in-process baseline.  `occupancy` (host, optional) receives hipOccupancyMaxActiveBlocksPerMultiprocessor of the launched
 * instantiation at its launch configuration.  What tests/test_gpu_lookup_split.py checks against fp64. */
typedef struct {
    int32_t n_pairs, H8, W8;    /* M = n_pairs * H8 * W8 pixels; H8, W8 >= 8 */
    int32_t variant;            /* 0 or 1 */
    const float* corr[4];       /* pyramid level l: [M, H8>>l, W8>>l] fp32 */
    const float* flow;          /* [M, 2] fp32 (x, y) */
    const void* weights;        /* [256, 768] 16-bit units */
    const int32_t* scale;       /* device: E8M0 byte of 2^-11 / sw */
    const float* bias;          /* [256] */
    void* out;                  /* [M, 512] 16-bit units: fp16 x 256 | correction bytes x 512 */
    int32_t* occupancy;         /* host, optional */
} vtgb_raft_lookup_convc1_args;
int vtgb_raft_lookup_convc1(const vtgb_raft_lookup_convc1_args* a, vtgb_stream_t stream);

/* Unit-level surface of vtgb_raft_update's SepConvGRU gate launches at VTGB_F16C8 / VTGB_BF16X3 (update.py:39-65): ONE half-step (half 0: the horizontal
 * 1x5 convolutions, half 1: the vertical 5x1 ones), launched by the function the refinement loop itself calls (csrc/raft_x3.hip x3_gru_half), on the
 * caller's buffers.  Pair rows are [M, 256 16-bit units] of 128 channels in the format `fmt` (vtgb_pair_pack), M = n_images * H8 * W8.
 *   stage 0 -- the z | r launch: pre = conv([h | x], w_zr) + start_zr (256 in, 256 out); z = sigmoid(pre[:, :128]) -> `z` fp32 [M, 128];
 *              sigmoid(pre[:, 128:]) * h -> `rh` as a pair row, h = the value its pair decodes to.  `h` and `x` are only read.
 *   stage 1 -- the q launch: pre = conv([rh | x], w_q) + start_q (256 in, 128 out); h' = (1 - z) h + z tanh(pre), read from and written IN PLACE to the
 *              pair `h_q` (which may be `h`).  `rh`, `z` and `x` are only read.
 *   stage 2 -- both, in that order.
 * x = [motion(126) | flow(2)]; the start maps are the loop-invariant `inp` third of the convolutions plus their bias, fp32.  w_zr / w_q are packed exactly
 * as vtgb_raft_update's table entries [10 + 4 half] / [12 + 4 half]; scale_zr / scale_q (VTGB_F16C8 only, ignored otherwise) are DEVICE int32: the E8M0
 * byte of 2^-11 / sw of that convolution.  Operands of a launch the stage does not run may be NULL.  The zero page of the out-of-image taps is the
 * library's own (allocated once per process), as in vtgb_pair_conv.  VTGB_EINVAL on the host, before any launch, for NULL args, a NULL operand of a
 * launch that runs, a bad fmt / half / stage, n_images < 1 or H8, W8 < 8, a missing scale at VTGB_F16C8.  What tests/test_gpu_gru_half.py checks
 * against fp64 (tests/gru_ref.py). */
typedef struct {
    int32_t fmt;                /* VTGB_F16C8 or VTGB_BF16X3 */
    int32_t n_images, H8, W8;   /* M = n_images * H8 * W8 pixels; H8, W8 >= 8 */
    int32_t half;               /* 0: 1x5, 1: 5x1 */
    int32_t stage;              /* 0: z | r launch, 1: q launch, 2: both */
    const void* h;              /* pair rows [M, 256]: read by stage 0 */
    void* h_q;                  /* pair rows [M, 256]: read and updated in place by stage 1 */
    const void* x;              /* pair rows [M, 256] */
    void* rh;                   /* pair rows [M, 256]: written by stage 0, read by stage 1 */
    float* z;                   /* [M, 128]: written by stage 0, read by stage 1 */
    const float* start_zr;      /* [M, 256] */
    const float* start_q;       /* [M, 128] */
    const void* w_zr;           /* [256, K] 16-bit units */
    const void* w_q;            /* [128, K] 16-bit units */
    const int32_t* scale_zr;    /* device */
    const int32_t* scale_q;     /* device */
} vtgb_raft_gru_half_args;
int vtgb_raft_gru_half(const vtgb_raft_gru_half_args* a, vtgb_stream_t stream);

/* Unit-level surface of RAFT's implicit-GEMM convolution launches at VTGB_BF16X3, VTGB_BF16 and VTGB_F32 (every RAFT convolution that is not an f16c8
 * launch): ONE launch_conv_gemm on the caller's buffers, its descriptor built by the helpers the production callers use (csrc/conv_descs.h: enc_conv /
 * enc_stem_conv of vtgb_raft_encoder for site 0, x3_conv / conv_desc of vtgb_raft_update for site 1), plus the moments finish when `moments` is given.
 *   out[m][n] = act(sum over taps (ty, tx) and channels c of x[img][oy * stride + ty - KH/2][ox * stride + tx - KW/2][c] * w[n][ty][tx][c] + bias[n])
 * over NHWC rows, m = (img * H + oy) * W + ox on the H x W OUTPUT grid; the input grid is Hi x Wi (0 = the output grid), out-of-image taps read zeros
 * (the library's own zero page, allocated once per process, as in vtgb_pair_conv).  Even kernels pad KH/2 before and KH/2 - 1 behind (the 4 x 1 stem GEMM
 * over the packed rows: taps oy - 2 .. oy + 1).  x = C1 channels from `a` (+ C2 more from `a2`: a virtual concatenation), contiguous rows:
 *   VTGB_BF16X3: bf16 pair rows [hi(C) | lo(C)] (vtgb_pair_pack), weights [N, taps, 3 (C1 + C2)] bf16 with the blocks [Wh | Wh | Wl] per source;
 *   VTGB_BF16: bf16 rows [C], weights [N, taps, C1 + C2] bf16;   VTGB_F32: fp32 rows, fp32 weights -- all in the kernels' K order (64-channel chunk
 *   major, tap minor), as the production tables pack them.
 * site 0 (encoders): K x K or the 4 x 1 stem, one source, stride 1 or 2.  site 1 (update block): KH x KW, one or two sources, stride 1; at VTGB_BF16 /
 * VTGB_F32 a 1 x 1 convolution is the plain GEMM the update block launches (out_scale applies there: mask.2's 0.25).
 * out_kind: VTGB_CONV_OUT_F32 fp32 rows [M, ld_out]; VTGB_CONV_OUT_PAIR_BF16 / _PAIR_F16C8 (VTGB_BF16X3 only): pair rows [M, 2 ld_out] 16-bit units, the
 * lo half at unit ld_out; VTGB_CONV_OUT_BF16 (VTGB_BF16 only): bf16 rows [M, ld_out], optionally out = [relu](act(.) + resid) (a ResidualBlock's tail,
 * resid bf16 rows [M, ld_resid]) or, with tail_w ([32, 256] bf16, N == 256), tail_out [M, 32] fp32 = act(.) as bf16 times tail_w^T instead of `out`.
 * moments (site 0, fp32 rows, H * W >= 256, N <= 128): [n_images, N, 2] fp32 = per image and channel the (sum, sum of squares) of the stored values, by the
 * epilogue's per-tile slots and launch_stats_finish_tiles as the encoders chain them; stats_part: scratch of >= (M / 256 + 2) * 128 * 4 floats (the
 * encoders' sizing), stats_part_floats its size.
 * Not expressible here: the gate epilogues (EPI_X3ZR / EPI_X3Q: vtgb_raft_gru_half), the unfused bf16 GRU (EPI_GRU, gate_from, frag_out / init_frag: reachable
 * only with the fused GRU kernel switched off by a debug hook) and raft_stem_pack_kernel (the caller provides the packed rows).
 * VTGB_EINVAL on the host, before any launch, for NULL args, a NULL operand, a bad dtype / out_kind / site / act / stride, non-positive sizes, C1 or C2
 * not a multiple of 64, a geometry the site does not have, an out_kind the dtype does not have, resid / tail_w / out_scale outside their out_kind,
 * moments with H * W < 256, a non-fp32 output, site 1 or a short stats_part.  What launch_conv_gemm refuses keeps its own code and message.  What
 * tests/test_gpu_conv_launch.py checks against fp64 (tests/conv_ref.py). */
#define VTGB_CONV_OUT_F32 0
#define VTGB_CONV_OUT_PAIR_BF16 1
#define VTGB_CONV_OUT_PAIR_F16C8 2
#define VTGB_CONV_OUT_BF16 3
typedef struct {
    int32_t dtype;              /* VTGB_F32, VTGB_BF16 or VTGB_BF16X3 */
    int32_t out_kind;           /* VTGB_CONV_OUT_* */
    int32_t site;               /* 0: encoder builders, 1: update-block builders */
    int32_t n_images, H, W;     /* output grid: M = n_images * H * W rows */
    int32_t KH, KW, stride;     /* stride 1 or 2 */
    int32_t Hi, Wi;             /* input grid; 0 = H, W */
    int32_t C1, C2;             /* channels per source (multiples of 64; C2 = 0: one source) */
    int32_t N;                  /* output channels */
    int32_t act;                /* 0 none, 1 relu, 2 sigmoid */
    int32_t post_relu;          /* with resid */
    float out_scale;            /* 0 = 1 */
    const void* a;
    const void* a2;
    const void* weights;
    const float* bias;          /* [N] or NULL */
    void* out;
    int64_t ld_out;             /* >= N; pair rows: 16-bit units per half */
    float* moments;             /* [n_images, N, 2] or NULL */
    float* stats_part;
    int64_t stats_part_floats;
    const void* resid;          /* VTGB_CONV_OUT_BF16: bf16 rows [M, ld_resid] or NULL */
    int64_t ld_resid;
    const void* tail_w;         /* VTGB_CONV_OUT_BF16: [32, 256] bf16 or NULL */
    float* tail_out;            /* [M, 32] */
} vtgb_conv_launch_args;
int vtgb_conv_launch(const vtgb_conv_launch_args* a, vtgb_stream_t stream);

/* Unit-level surface of vtgb_raft_encoder's stem (extractor.py:128-130: 7x7, stride 2, 3 -> 64 channels on x - 127.5 as a bf16 pair) at VTGB_BF16X3 --
 * also the stem of VTGB_F16C8 -- launched by the function the encoder itself calls (csrc/raft_enc.hip enc_stem_x3), through the caller's workspace.
 *   variant 1: the fused kernel the encoder launches at the sizes it takes (H, W even, 16 <= W / 2 <= 112, H / 2 >= 4): the packed rows are built in LDS
 *              from the raw frames and multiplied there (csrc/conv64.hip stem7x7_kernel, split-operand form); VTGB_EUNSUPPORTED for other sizes;
 *   variant 2: what the encoder launches for fnet (VTGB_CONV_OUT_F32, H/2 * W/2 >= 256, variant 1's sizes): variant 1's rows, and the moments added per
 *              256-row tile in the order of variant 0's GEMM epilogue by a pass of their own -- variant 0's moments bit for bit;
 *   variant 0: the route it replaced and the encoder's fallback for other sizes: raft_stem_pack_kernel (a 128-channel hi | lo image in the workspace) +
 *              the 4 x 1 implicit GEMM over it (+ the pair pass for pair rows).
 * All accumulate every output element in the same order (bias, then K in the table's order): their fp32 rows are bit-identical.
 * frames [n_images, 3, H, W] fp32; weights = the encoder table's entry [0] at VTGB_BF16X3, [64, 768] bf16 ([Wh | Wh | Wl] chunks of 4 x 64), bias = [1].
 * out_kind VTGB_CONV_OUT_F32 (fnet): out = fp32 rows [n_images * H/2 * W/2, 64], moments [n_images, 64, 2] = per image and channel the (sum, sum of
 *   squares) of the stored values, added in a fixed order (variant 1: per run of rows; variants 0, 2: per 256-row tile -- the last bits of 1 may differ);
 * VTGB_CONV_OUT_PAIR_BF16 / _PAIR_F16C8 (cnet, BatchNorm folded): out = relu(.) as pair rows [., 128 16-bit units] (vtgb_pair_pack's layout, lo half at unit 64).
 * VTGB_EINVAL on the host, before any launch, for NULL args, bad dims / variant / out_kind, a NULL operand or one that is not 16-byte aligned;
 * VTGB_EWORKSPACE for a NULL or short workspace.  What tests/test_gpu_stem_x3.py checks. */
typedef struct {
    int32_t n_images, H, W;
    int32_t variant;            /* 0: pack + implicit GEMM, 1: fused, 2: fused + tile-order moments */
    int32_t out_kind;           /* VTGB_CONV_OUT_F32, VTGB_CONV_OUT_PAIR_BF16 or VTGB_CONV_OUT_PAIR_F16C8 */
    const float* images;        /* [n_images, 3, H, W] */
    const void* weights;        /* [64, 768] bf16 */
    const float* bias;          /* [64] */
    void* out;
    float* moments;             /* VTGB_CONV_OUT_F32: [n_images, 64, 2]; else ignored (may be NULL) */
    void* workspace;
    size_t workspace_bytes;
} vtgb_raft_stem_args;
size_t vtgb_raft_stem_workspace_bytes(const vtgb_raft_stem_args* a);
int vtgb_raft_stem(const vtgb_raft_stem_args* a, vtgb_stream_t stream);

/* Unit-level surface of ONE layer1 convolution of vtgb_raft_encoder at VTGB_F16C8 (extractor.py:136-143: 3x3, stride 1, 64 -> 64 channels at half resolution;
 * added at version 601 without a bump), launched by the function the encoder itself calls (csrc/raft_enc.hip enc_conv_h8), through the caller's workspace.
 *   variant 0: the implicit GEMM of csrc/gemm_h8.hip on its 64-wide tile -- every pixel's 256 bytes staged once per tap;
 *   variant 1: the row-resident kernel (csrc/conv64.hip layer1_h8_kernel; 16 <= W <= 112, H >= 4, else VTGB_EUNSUPPORTED): every input row staged once into
 *              an LDS ring, the weights in registers, the taps as shifted fragment reads.  It writes no moments;
 *   variant 2: (VTGB_CONV_OUT_F32, H * W >= 256) variant 1's rows, and the moments added per 256-row tile in the order of variant 0's epilogue by a pass of
 *              their own -- variant 0's moments bit for bit.
 * Every output element is accumulated in one order -- the bias, the nine fp16 k-tiles in tap order, the nine correction k-tiles -- so the variants' rows are
 * bit-identical.  x: f16c8 pair rows [n_images * H * W, 128 16-bit units] (vtgb_pair_pack); weights / bias / scale: the encoder table's entries of the
 * convolution ([64, 1152] 16-bit units, [64] fp32, one int32 of weights[40]).
 * out_kind VTGB_CONV_OUT_F32 (fnet): out = fp32 rows [M, 64]; moments (variants 0, 2; H * W >= 256; NULL = none) [n_images, 64, 2] = per image and channel
 *   the (sum, sum of squares) of the stored values;
 * VTGB_CONV_OUT_PAIR_F16C8 (cnet, BatchNorm folded): out = relu(.) as pair rows [M, 128 units], or with resid (f16c8 pair rows [M, 128]) the ResidualBlock's
 *   tail relu(resid + relu(.)); VTGB_CONV_OUT_PAIR_BF16: that tail as a bf16 pair (resid required).
 * VTGB_EINVAL on the host, before any launch, for NULL args, bad dims / variant / out_kind, resid or moments outside their out_kind, moments with variant 1 or
 * H * W < 256, variant 2 without them, a NULL operand or a misaligned one (16 bytes; scale: 4); VTGB_EWORKSPACE for a NULL or short workspace.  What
 * tests/test_gpu_layer1_h8.py checks. */
typedef struct {
    int32_t n_images, H, W;     /* the convolution's own grid */
    int32_t variant;            /* 0: implicit GEMM, 1: row-resident kernel, 2: row-resident kernel + tile-order moments */
    int32_t out_kind;           /* VTGB_CONV_OUT_F32, VTGB_CONV_OUT_PAIR_BF16 or VTGB_CONV_OUT_PAIR_F16C8 */
    const void* x;              /* [n_images * H * W, 128] 16-bit units */
    const void* weights;        /* [64, 1152] 16-bit units */
    const float* bias;          /* [64] */
    const int32_t* scale;       /* the E8M0 byte of the weights' scale */
    const void* resid;          /* pair rows only: f16c8 pair rows [M, 128] or NULL */
    void* out;
    float* moments;             /* VTGB_CONV_OUT_F32, variants 0 / 2: [n_images, 64, 2] or NULL */
    void* workspace;
    size_t workspace_bytes;
} vtgb_raft_layer1_h8_args;
size_t vtgb_raft_layer1_h8_workspace_bytes(const vtgb_raft_layer1_h8_args* a);
int vtgb_raft_layer1_h8(const vtgb_raft_layer1_h8_args* a, vtgb_stream_t stream);

/* CorrBlock.__init__ (raft_utils/corr.py:12-27; the all-pairs product :52-60): for every pair the correlation of each
 * pixel of image 1 with every pixel of image 2 over the `dim` = 256 features, divided by sqrt(dim), and its three
 * avg_pool2d(2, stride 2) -- one kernel, the four levels are its only output.  Pair n uses the feature maps of images
 * (n / pairs_per_clip) * frames_per_clip + n % pairs_per_clip + {first_off, second_off}: consecutive frames of whole
 * clips are (T-1, T, 0, 1); separate image1 / image2 batches of N encoded as cat([image1, image2]) are (N, N, 0, N).
 * VTGB_BF16: half-precision MFMA on an fp16 copy of the features (made in the workspace), fp32 accumulate and scale,
 * levels IEEE half; VTGB_F32: fp32 FMAs, levels fp32; VTGB_BF16X3: the features as bf16 pairs (hi | lo planes in the workspace),
 * three bf16 MFMA products per fp32 product, fp32 accumulate, levels fp32. */
typedef struct {
    int32_t dtype, n_pairs, H8, W8, dim;
    int32_t pairs_per_clip, frames_per_clip, first_off, second_off, n_images;
    float scale;                /* 1 / sqrt(dim) = 1/16                                                            */
    const float* fmap;          /* [n_images, H8*W8, dim] fp32 (vtgb_raft_encoder output)                           */
    void* levels[4];            /* level l: [n_pairs*H8*W8, H8>>l, W8>>l] half (VTGB_BF16) or fp32 (VTGB_F32, VTGB_BF16X3) */
    void* workspace;
    size_t workspace_bytes;
} vtgb_raft_corr_args;
size_t vtgb_raft_corr_workspace_bytes(const vtgb_raft_corr_args* a);
int vtgb_raft_corr(const vtgb_raft_corr_args* a, vtgb_stream_t stream);

/* RAFT BasicEncoder (raft_utils/extractor.py:116-189): stem 7x7/2, six ResidualBlocks, 1x1 head; the input
 * scaling 2*(x/255)-1 of RAFT.forward (xraft.py:105-106) is applied inside.  norm = 0: InstanceNorm2d (fnet);
 * norm = 1: the caller has folded the eval-mode BatchNorm2d that follows every convolution into the packed
 * weights and biases (cnet).  Output: NHWC features [n_images * H/8 * W/8, 256] fp32.
 * weights (`dtype`): [0] conv1.weight: the stem as a 4x1 convolution over the 2x2 space-to-depth image, channel =
 *   dX*12 + py*6 + px*3 + c (48, zero-padded to 64), ky = 2 tY + py - 1, kx = 2 dX + px - 1.  VTGB_F32: [64, 4 (tY), 64], unscaled
 *   (the kernel packs 2*(x/255)-1 itself).  VTGB_BF16: [64, 2 (chunk), 4 (tY), 64] = the same table twice, scaled by 2/255: the
 *   kernel feeds x - 127.5 to the GEMM as a bf16 pair, chunk 0 = hi = bf16(v), chunk 1 = lo = bf16(v - hi), so float-valued
 *   (CLIP-normalised) frames keep 16 significant bits (since version 300; 210 fed hi alone) [1] conv1.bias; per block b (layer1.0, 1.1, 2.0, 2.1, 3.0, 3.1) at
 *   2 + 6 b: conv1.weight [C, 3,3,Cin_pad] , conv1.bias, conv2.weight [C, 3,3,C_pad], conv2.bias,
 *   downsample.0.weight [C, Cin_pad] or NULL, downsample.0.bias or NULL  (96-channel stages: C_pad = 128, zero-filled; with norm = 1 the
 *   OUTPUT rows and biases of those stages are padded to C_pad as well: the GEMM stores the activations directly);
 *   [38] conv2.weight [256, 128] [39] conv2.bias */
#define VTGB_RAFT_ENC_NW 40
typedef struct {
    int32_t dtype, n_images, H, W, norm;
    const float* images;        /* [n_images, 3, H, W] fp32 */
    const void* const* weights; /* host array              */
    float* out;                 /* [n_images * H/8 * W/8, 256] fp32 */
    void* workspace;
    size_t workspace_bytes;
} vtgb_raft_encoder_args;
size_t vtgb_raft_encoder_workspace_bytes(const vtgb_raft_encoder_args* a);
int vtgb_raft_encoder(const vtgb_raft_encoder_args* a, vtgb_stream_t stream);

/* ---- LLM decode-step building blocks ("next" row) ----------------------------
 * The LLM itself is third-party on both sides (HF weights and GEMMs); these fuse the small
 * per-layer ops of a KV-cached greedy decode step with the exact rounding points of
 * transformers' modeling_llama (LlamaRMSNorm, apply_rotary_pos_emb, LlamaMLP).  `dtype` is the
 * activation dtype (VTGB_BF16 / VTGB_F32); `pos` is a DEVICE int64 (current position), so one
 * captured hipGraph serves every step.
 *   vtgb_llm_rmsnorm:          x[rows,H] (+= delta, written back if delta != NULL); h = w * norm(x)
 *   vtgb_llm_rope_cache:       qkv[B, nq+2nkv, hd] -> q_out[B,nq,hd] rotated; K/V cache [B,nkv,tmax,hd] row *pos (cos_t = sin_t = NULL: no rotary)
 *   vtgb_llm_rope_cache_prefill: qkv[B, S, (nq+2nkv)*hd]: q and k of every position rotated IN PLACE, k / v copied to cache rows 0..S-1
 *   vtgb_llm_decode_attention: out[B, nq*hd] = softmax(scale q K[0..*pos]^T) V[0..*pos]
 *   vtgb_llm_silu_mul:         act[rows, I] = silu(gu[:, :I]) * gu[:, I:]                       */
int vtgb_llm_rmsnorm(int dtype, void* x, const void* delta, const void* w, void* h, int64_t rows, int32_t H, float eps,
                     vtgb_stream_t stream);
int vtgb_llm_rope_cache(int dtype, const void* qkv, void* q_out, void* kc, void* vc, const void* cos_t, const void* sin_t,
                        const int64_t* pos, int32_t B, int32_t nq, int32_t nkv, int32_t hd, int32_t tmax, vtgb_stream_t stream);
int vtgb_llm_rope_cache_prefill(int dtype, void* qkv, void* kc, void* vc, const void* cos_t, const void* sin_t, int32_t B, int32_t S, int32_t nq,
                                int32_t nkv, int32_t hd, int32_t tmax, vtgb_stream_t stream);
int vtgb_llm_decode_attention(int dtype, const void* q, const void* kc, const void* vc, void* out, const int64_t* pos, int32_t B,
                              int32_t nq, int32_t nkv, int32_t hd, int32_t tmax, float scale, vtgb_stream_t stream);
int vtgb_llm_silu_mul(int dtype, const void* gu, void* act, int64_t rows, int32_t I, vtgb_stream_t stream);

/* The seq2seq language model of the BLIP-2 flavours (Flan-T5 under `language_model.generate`: eval/utils/model.py:427-437,
 * src/models/components/xblip2.py:1553-1556) with transformers' modeling_t5 arithmetic: T5LayerNorm = vtgb_llm_rmsnorm (no mean, no
 * bias), projections = vtgb_gemm / vtgb_gemm_skinny, cache append = vtgb_llm_rope_cache with cos_t = sin_t = NULL, and
 *   vtgb_llm_attention_rows: out[r, h, :] = softmax_k(scale q[r, h] . k[b, h, key] + bias[qpos, h, key]) v[b, h, key, :] over independent
 *     query rows r (b = r / rows_per_batch).  Keys [0, n_keys), or [0, *pos] with bias row *pos when `pos` (a DEVICE int64) is given --
 *     the decoder's self-attention over its static cache; pos == NULL: query position r % rows_per_batch -- the encoder's
 *     self-attention (rows = B x P, token-major q|k|v) and the decoder's cross-attention (bias NULL).  All strides in elements;
 *     heads are `head_dim` apart in q / out; `bias` has the activation dtype; scores and weights are rounded to it where HF does
 *     (softmax itself in fp32).  t_pad >= the largest key count (sizes the kernel's score buffer).
 *   vtgb_llm_gated_act: act[r, i] = f(gu[r, i]) (* gu[r, I + i] if gated); kind 0 SiLU, 1 gelu_new (Flan-T5's gated-gelu), 2 ReLU, 3 erf-GELU */
typedef struct {
    int32_t dtype, rows, heads, head_dim, rows_per_batch, n_keys, t_pad;
    float scale;
    const void* q;   int64_t q_row;
    const void* k;   const void* v;   int64_t kv_batch, kv_head, kv_tok;
    const void* bias; int64_t bias_pos, bias_head;
    const int64_t* pos;
    void* out;       int64_t o_row;
} vtgb_llm_attn_rows_args;
int vtgb_llm_attention_rows(const vtgb_llm_attn_rows_args* a, vtgb_stream_t stream);
int vtgb_llm_gated_act(int dtype, const void* gu, void* act, int64_t rows, int32_t I, int32_t kind, int32_t gated, vtgb_stream_t stream);

/* Skinny GEMM of the decode step: out[M, N] = x[M, K] . w[N, K]^T, bf16 operands, M <= 128 (one token per
 * clip), K a multiple of 64 -- what `F.linear(h, weight)` (hipBLASLt) computes under `language_model.generate`
 * (eval/utils/model.py:223-233; transformers LlamaDecoderLayer's q/k/v/o/gate/up/down projections and lm_head).  The weights
 * stream from HBM once: one workgroup per (128-row weight tile, K split) -- `n_splits` splits (0 = chosen by the library) where
 * the tiles alone would leave CUs without a stream.  Without a split the tile is rounded and stored straight to `out` (no
 * workspace: vtgb_gemm_skinny_workspace_bytes returns 0).  With a split every workgroup leaves an fp32 fragment in `workspace`
 * (n_tiles * n_splits * M * 128 * 4 bytes) and a second launch adds a tile's fragments in split order and rounds once to
 * `out_dtype` (deterministic: no atomics). */
typedef struct {
    int32_t M, N, K, n_splits;
    const void* x; int64_t ldx;          /* bf16 [M, K] */
    const void* w; int64_t ldw;          /* bf16 [N, K] (nn.Linear.weight) */
    void* out; int64_t ldo;              /* [M, N] */
    int32_t out_dtype;                   /* VTGB_BF16 | VTGB_F32 */
    int32_t w_tiled;                     /* 1: `w` was prepared by vtgb_pack_skinny_weight (ldw ignored): every (128-row tile, 64-deep
                                            k-tile) is one contiguous 16 KiB block in the kernel's LDS order -- 1 KiB reads instead of
                                            eight 128-byte row segments a DRAM page apart */
    void* workspace;
    size_t workspace_bytes;
    int32_t defer_reduce;                /* 1 (with a K split): skip the second launch -- `out` is not written; the consumer adds the fragments
                                            workspace[(tile * n_splits + split) * M + m][128] in split order and rounds once itself
                                            (vtgb_llm_rmsnorm_parts, vtgb_llm_rope_cache_parts; vtgb_gemm_skinny_splits tells n_splits) */
} vtgb_gemm_skinny_args;
int32_t vtgb_gemm_skinny_splits(const vtgb_gemm_skinny_args* a);   /* the K split the call will use (1: `out` is written directly) */
/* The decode step's consumers of a deferred split (bf16; rows = the GEMM's M <= 128): x += sum of the fragments (rounded once, as the reduce
 * launch would have stored it), h = rmsnorm(x) * w;  and rotary + cache append reading q | k | v from the fragments.  Same values as the two-launch
 * form, bit for bit (tests/test_decode.py). */
int vtgb_llm_rmsnorm_parts(int dtype, void* x, const float* part, int32_t n_splits, const void* w, void* h, int64_t rows, int32_t H, float eps,
                           vtgb_stream_t stream);
int vtgb_llm_rope_cache_parts(int dtype, const float* part, int32_t n_splits, void* q_out, void* kc, void* vc, const void* cos_t, const void* sin_t,
                              const int64_t* pos, int32_t B, int32_t nq, int32_t nkv, int32_t hd, int32_t tmax, vtgb_stream_t stream);

/* ---- Padded prompt batches on the graph decoders (HF generate with an attention mask; transformers'
 * GenerationMixin._prepare_position_ids_for_generation / _update_model_kwargs_for_generation, modeling_t5's extended mask).
 * New entries next to the unpadded ones, which are unchanged; all per-row data is DEVICE memory, so one captured graph serves
 * every ragged batch of one shape.
 *   vtgb_llm_rope_cache_pos / _parts_pos: vtgb_llm_rope_cache / _parts with the rotary row of batch entry b = *pos + rope_off[b]
 *     (rope_off [B] int64; HF: position_ids[b, P-1] + step); the cache row stays *pos.  rope_off == 0: the same values bit for bit.
 *   vtgb_llm_rope_cache_prefill_pos: vtgb_llm_rope_cache_prefill with the rotary row of (b, s) = pos_ids[b, s] (pos_ids [B, S] int64;
 *     HF: attention_mask.cumsum(-1) - 1, pads at 0).  Rows are clamped to [0, tmax).
 *   vtgb_llm_decode_attention_masked: vtgb_llm_decode_attention over the keys [0, *pos] with key_valid[b, key] != 0 (key_valid
 *     [B, tmax] uint8).  Masked keys get no weight and neither their K nor their V row is read (a pad slot may hold anything,
 *     NaN included); the valid keys are summed in the unmasked order.  No valid key: the output row is 0.
 *   vtgb_llm_attention_rows_masked: vtgb_llm_attention_rows with key_valid[(r / rows_per_batch) * key_valid_batch_stride + key]
 *     (uint8) -- the T5 encoder's self-attention and the decoder's cross-attention over a padded encoder input.
 * The prefill's attention is vtgb_attention with key_mask = finfo(float32).min on pad keys and causal = 1 (finite rows also
 * where a query has no valid key). */
int vtgb_llm_rope_cache_pos(int dtype, const void* qkv, void* q_out, void* kc, void* vc, const void* cos_t, const void* sin_t,
                            const int64_t* pos, const int64_t* rope_off, int32_t B, int32_t nq, int32_t nkv, int32_t hd, int32_t tmax,
                            vtgb_stream_t stream);
int vtgb_llm_rope_cache_parts_pos(int dtype, const float* part, int32_t n_splits, void* q_out, void* kc, void* vc, const void* cos_t,
                                  const void* sin_t, const int64_t* pos, const int64_t* rope_off, int32_t B, int32_t nq, int32_t nkv, int32_t hd,
                                  int32_t tmax, vtgb_stream_t stream);
int vtgb_llm_rope_cache_prefill_pos(int dtype, void* qkv, void* kc, void* vc, const void* cos_t, const void* sin_t, const int64_t* pos_ids,
                                    int32_t B, int32_t S, int32_t nq, int32_t nkv, int32_t hd, int32_t tmax, vtgb_stream_t stream);
int vtgb_llm_decode_attention_masked(int dtype, const void* q, const void* kc, const void* vc, void* out, const int64_t* pos,
                                     const uint8_t* key_valid, int32_t B, int32_t nq, int32_t nkv, int32_t hd, int32_t tmax, float scale,
                                     vtgb_stream_t stream);
int vtgb_llm_attention_rows_masked(const vtgb_llm_attn_rows_args* a, const uint8_t* key_valid, int64_t key_valid_batch_stride,
                                   vtgb_stream_t stream);

/* ---- Split-KV decode attention (attn_decode.hip): vtgb_llm_decode_attention{,_masked} for long caches and grouped-query heads.
 *   out[B, nq*hd] = softmax(scale q K[0..*pos]^T) V[0..*pos] over the static cache kc / vc [B, nkv, tmax, hd], query head h reading K/V
 *   head h / (nq / nkv) in place.  key_valid [B, tmax] uint8 or NULL (every key valid).  Limits: hd 64 or 128, tmax a multiple of 64 up
 *   to 16384, nq % nkv == 0 (VTGB_EINVAL otherwise), q / kc / vc / out / workspace 16-byte aligned; anything else is VTGB_EUNSUPPORTED
 *   on the host, before any launch.  `dtype` VTGB_BF16 / VTGB_F32; scores, softmax weights and sums are fp32.
 * Two launches, no atomics.  Pass 1: one workgroup per (chunk of 256 consecutive keys, K/V head x block of up to 8 of its query heads,
 *   batch row) -- the grid depends on tmax only and a workgroup whose chunk starts past *pos leaves at once, so one captured graph serves
 *   every step; K/V of a chunk are read once for all the query heads of the block.  It leaves fp32 partials per (row r = b * nq + head,
 *   chunk c) in `workspace`, NC = ceil(tmax / 256):
 *     float O [B * nq][NC][hd]   O[r][c][:] = sum over the chunk's visible keys of exp(s - m) v
 *     float ml[B * nq][NC][2]    m = the largest scaled score s of the chunk's visible keys (-inf: none), l = sum exp(s - m)
 *   = vtgb_llm_decode_attention_split_workspace_bytes = B * nq * NC * (hd + 2) * 4 bytes (0 for an empty shape).
 *   Pass 2, per row: M = max_c m_c, w_c = exp(m_c - M), out = (sum_c w_c O_c) / (sum_c w_c l_c) over the chunks 0 .. *pos / 256 in
 *   ascending order, rounded once to `dtype`; a chunk without a visible key has weight 0.
 * Visible keys: key <= *pos and key_valid[b, key] != 0.  Nothing past *pos is read; the K and V values of a masked key never enter a
 *   product (weight exactly 0), so a pad slot may hold anything, NaN included.  No visible key: the output row is 0.
 * Which keys share a partial sum and the order inside every sum depend on the key index, dtype and hd only: a row's bits do not depend on
 *   B, tmax, nq / nkv or the other rows (they differ from vtgb_llm_decode_attention's in the last bits: another summation order). */
int64_t vtgb_llm_decode_attention_split_workspace_bytes(int32_t B, int32_t nq, int32_t hd, int32_t tmax);
int vtgb_llm_decode_attention_split(int dtype, const void* q, const void* kc, const void* vc, void* out, const int64_t* pos,
                                    const uint8_t* key_valid /* NULL: none */, void* workspace, int32_t B, int32_t nq, int32_t nkv, int32_t hd,
                                    int32_t tmax, float scale, vtgb_stream_t stream);

/* ---- fp8 K/V cache of the Llama decode step (opt-in: kv_cache = "fp8"; attn_decode.hip, llm.hip).  Every K row (after rotary) and every V
 *   row -- one token of one K/V head, hd values -- is stored as OCP e4m3fn codes and one power-of-two scale:
 *     uint8 kc8 / vc8 [B, nkv, tmax, hd]    float ks / vs [B, nkv, tmax]
 *   scale = 2^e, e = the smallest integer with amax * 2^-e <= 448 (from the binary exponent; 0 for a zero row), clamped below at -100;
 *   codes = row * 2^-e rounded to nearest even (ops.quantize_fp8_kv is the definition; the writers reproduce it bit for bit).  code * scale
 *   is exactly a bf16 number: the mode is a bf16 model whose K/V pass through that rounding as they are produced.  Non-finite K/V are
 *   outside the contract.  Activations are VTGB_BF16 (any other dtype: VTGB_EINVAL); hd 64 or 128 (VTGB_EUNSUPPORTED otherwise).
 * vtgb_llm_decode_attention_split_fp8: vtgb_llm_decode_attention_split over that cache.  Same q / out layout, key_valid, visibility rules
 *   (nothing past *pos is read, codes or scales; a masked or stale slot may hold anything, the e4m3 NaN code and NaN scales included),
 *   workspace (vtgb_llm_decode_attention_split_workspace_bytes), pass 2, limits and error codes: VTGB_EINVAL for a NULL operand, a
 *   non-positive size, nq % nkv != 0 or a dtype other than VTGB_BF16; VTGB_EUNSUPPORTED for hd outside {64, 128}, tmax not a multiple of
 *   64 up to 16384, q / kc8 / vc8 / out / workspace not 16-byte or ks / vs not 4-byte aligned -- on the host, before any launch.
 *   The output equals, BIT FOR BIT, vtgb_llm_decode_attention_split(VTGB_BF16) on the dequantised cache (kc = kc8 * ks, vc = vc8 * vs):
 *   the same partition of every sum, the scales applied as exact power-of-two factors (to a row's score, to its softmax weight).
 * vtgb_llm_rope_cache_fp8: the decode step's rotary + append (vtgb_llm_rope_cache and its _parts / _pos forms in one args struct).
 *   q_out: the bits of the existing entries; the K row after rotary (rounded to bf16 as there) and the V row are quantised into row *pos
 *   of kc8 / ks and vc8 / vs (*pos outside [0, tmax): no cache write).  Exactly one of qkv and part (VTGB_EINVAL otherwise).
 * vtgb_llm_rope_cache_prefill_fp8: vtgb_llm_rope_cache_prefill{,_pos} (pos_ids NULL: the rotary row of position s is s): q and k rotated
 *   in place, codes and scales of rows 0 .. S-1 written, and the DEQUANTISED k and v written back in place into qkv, so that the prefill
 *   attention attends over the values the decode steps will read. */
typedef struct {
    int32_t dtype;                       /* VTGB_BF16 */
    int32_t B, nq, nkv, hd, tmax;
    int32_t n_splits;                    /* with `part`: > 1 */
    const void* qkv;                     /* bf16 [B, (nq + 2 nkv) * hd], or NULL with `part` */
    const float* part;                   /* the deferred K-split fragments of the q|k|v projection (vtgb_gemm_skinny, defer_reduce; B <= 128) */
    void* q_out;                         /* bf16 [B, nq * hd] */
    uint8_t* kc8; uint8_t* vc8;          /* [B, nkv, tmax, hd] */
    float* ks; float* vs;                /* [B, nkv, tmax] */
    const void* cos_t; const void* sin_t;/* bf16 [tmax, hd] */
    const int64_t* pos;                  /* device: the cache row */
    const int64_t* rope_off;             /* NULL, or [B]: the rotary row of batch entry b is *pos + rope_off[b] (padded batches) */
} vtgb_llm_rope_cache_fp8_args;
int vtgb_llm_rope_cache_fp8(const vtgb_llm_rope_cache_fp8_args* a, vtgb_stream_t stream);
int vtgb_llm_rope_cache_prefill_fp8(int dtype, void* qkv, uint8_t* kc8, uint8_t* vc8, float* ks, float* vs, const void* cos_t, const void* sin_t,
                                    const int64_t* pos_ids /* NULL: none */, int32_t B, int32_t S, int32_t nq, int32_t nkv, int32_t hd, int32_t tmax,
                                    vtgb_stream_t stream);
int vtgb_llm_decode_attention_split_fp8(int dtype, const void* q, const uint8_t* kc8, const uint8_t* vc8, const float* ks, const float* vs, void* out,
                                        const int64_t* pos, const uint8_t* key_valid /* NULL: none */, void* workspace, int32_t B, int32_t nq,
                                        int32_t nkv, int32_t hd, int32_t tmax, float scale, vtgb_stream_t stream);

/* ---- Beam search on the Llama decode step (opt-in: beam_search = "graph"; attn_decode.hip, beam.hip; added at version 601 without a bump).
 *   R = B * K beam rows; the beams of batch item b are the rows b K .. b K + K - 1.
 * vtgb_llm_decode_attention_beam: the split-KV decode attention with two K/V sources, so that re-ordering beams copies no K/V and the prompt's
 *   K/V exist once per batch item.  kp / vp [B, nkv, tmax_p, hd]: the prompt cache, as the prefill entries write it on B rows.  kg / vg
 *   [R, nkv, tmax_g, hd]: what the beams generate, row r appending at slot = the step.  src_row [R, tmax_g] int32: the generated-cache row that
 *   holds beam row r's key of slot s.  Key t of row r is kp[r / K, :, t] for t < *n_prompt, else kg[src_row[r, t - *n_prompt], :, t - *n_prompt];
 *   it is visible while t <= *pos and (prompt keys, with key_valid [B, tmax_p] uint8) key_valid[r / K, t] != 0.  *n_prompt and *pos are device
 *   int64 (one captured graph serves every prompt length of a bucket), clamped to [0, tmax_p] and to *n_prompt + tmax_g - 1; a table entry is
 *   clamped into [0, R) before use: a wrong table gives wrong numbers, never a read outside the caches.
 *   Chunks, waves, lanes and the order of every sum follow the global key index t as in vtgb_llm_decode_attention_split: the output equals, BIT
 *   FOR BIT, that entry's on the cache [R, nkv, T, hd] this gather materialises.  Nothing past *pos, no masked slot and no prompt slot
 *   >= *n_prompt reaches an output, NaN included.  Workspace: vtgb_llm_decode_attention_split_workspace_bytes at (R, nq, hd, tmax_p + tmax_g);
 *   pass 2 is that entry's.  VTGB_EINVAL: NULL args / operand, a dtype other than VTGB_BF16 / VTGB_F32, a non-positive size, R % K != 0,
 *   nq % nkv != 0; VTGB_EUNSUPPORTED: hd outside {64, 128}, tmax_p or tmax_g not a multiple of 64, tmax_p + tmax_g > 16384, a misaligned operand
 *   (16 bytes; src_row 4) -- on the host, before any launch.
 * vtgb_llm_beam_candidates: one step's logits [R, V] (`dtype`, as the lm_head leaves them) -> per batch item the 2 K best continuations.  Per
 *   row, in fp32: lp = (x - m) - log(sum exp(x - m)), m = max x; for every DISTINCT id in seq[r, 0 .. *step) (int64 [R, N], *step device int64
 *   clamped to [0, N], ids outside [0, V) ignored) lp = lp < 0 ? lp * penalty : lp / penalty (HF's RepetitionPenaltyLogitsProcessor on the
 *   log-probabilities); lp[eos] = -inf while *step < min_new (eos < 0: none); score = lp + running[r].  Per batch item the 2 K largest of its
 *   K * V scores in descending order: cand_score [B, 2 K] fp32, cand_idx [B, 2 K] int32 = k * V + token; equal scores in ascending index.
 *   The order of every sum is fixed by V alone: a row's lp bits do not depend on B, K or the row's place.  Workspace: R * V * 4 +
 *   R * 2 K * 8 bytes.  VTGB_EINVAL: NULL args / operand (seq may be NULL when N == 0), a bad dtype, non-positive R / K / V, R % K != 0,
 *   N < 0, penalty <= 0; VTGB_EUNSUPPORTED: 2 K > V, K > 16, V > 2^20, a workspace that is too small or not 16-byte aligned. */
typedef struct {
    int32_t dtype;                       /* VTGB_BF16 / VTGB_F32: q, the caches, out */
    int32_t R, K, nq, nkv, hd, tmax_p, tmax_g;
    float scale;
    const void* q;                       /* [R, nq * hd] */
    const void* kp; const void* vp;      /* [R / K, nkv, tmax_p, hd] */
    const void* kg; const void* vg;      /* [R, nkv, tmax_g, hd] */
    const int32_t* src_row;              /* [R, tmax_g] */
    void* out;                           /* [R, nq * hd] */
    const int64_t* n_prompt;             /* device */
    const int64_t* pos;                  /* device: the last visible key */
    const uint8_t* key_valid;            /* [R / K, tmax_p] or NULL */
    void* workspace;
} vtgb_llm_decode_attention_beam_args;
int vtgb_llm_decode_attention_beam(const vtgb_llm_decode_attention_beam_args* a, vtgb_stream_t stream);
/* vtgb_llm_decode_attention_beam_fp8 (opt-in: beam_search = "graph+kv8" with kv_cache = "fp8"; added at version 601 without a bump):
 *   vtgb_llm_decode_attention_beam over fp8 K/V caches in vtgb_llm_decode_attention_split_fp8's format.  kp8 / vp8 [B, nkv, tmax_p, hd] uint8
 *   e4m3 codes with kps / vps [B, nkv, tmax_p] fp32 power-of-two row scales: the prompt cache, as vtgb_llm_rope_cache_prefill_fp8 writes it on
 *   B = R / K rows.  kg8 / vg8 [R, nkv, tmax_g, hd] with kgs / vgs [R, nkv, tmax_g]: what the beams generate, row r appending at slot = the step
 *   (vtgb_llm_rope_cache_fp8).  src_row, *n_prompt, *pos, key_valid, the clamps, the workspace and pass 2 are vtgb_llm_decode_attention_beam's:
 *   key t of row r is row t of item r / K's prompt cache for t < *n_prompt, else row t - *n_prompt of generated-cache row
 *   clamp(src_row[r, t - *n_prompt], 0, R - 1), codes and scales from the same row.  An invisible key is loaded from row 0 of the item's prompt
 *   cache, its codes replaced by zeros and its scales by 1 before any product: nothing past *pos, no masked slot and no prompt slot >= *n_prompt
 *   reaches an output, whatever it holds (the e4m3 NaN code, a NaN scale, a table entry outside [0, R)).
 *   The partition of every sum is vtgb_llm_decode_attention_split_fp8's on the global key index: the output equals, BIT FOR BIT,
 *   vtgb_llm_decode_attention_beam(VTGB_BF16) on the dequantised caches, and so vtgb_llm_decode_attention_split on the gathered dequantised cache.
 *   VTGB_EINVAL: NULL args / operand, a dtype other than VTGB_BF16, a non-positive size, R % K != 0, nq % nkv != 0; VTGB_EUNSUPPORTED: hd outside
 *   {64, 128}, tmax_p or tmax_g not a multiple of 64, tmax_p + tmax_g > 16384, a misaligned operand (q / codes / out / workspace 16 bytes;
 *   scales and src_row 4) -- on the host, before any launch. */
typedef struct {
    int32_t dtype;                       /* VTGB_BF16: q, out */
    int32_t R, K, nq, nkv, hd, tmax_p, tmax_g;
    float scale;
    const void* q;                       /* [R, nq * hd] */
    const uint8_t* kp8; const uint8_t* vp8;  /* [R / K, nkv, tmax_p, hd] */
    const float* kps; const float* vps;  /* [R / K, nkv, tmax_p] */
    const uint8_t* kg8; const uint8_t* vg8;  /* [R, nkv, tmax_g, hd] */
    const float* kgs; const float* vgs;  /* [R, nkv, tmax_g] */
    const int32_t* src_row;              /* [R, tmax_g] */
    void* out;                           /* [R, nq * hd] */
    const int64_t* n_prompt;             /* device */
    const int64_t* pos;                  /* device: the last visible key */
    const uint8_t* key_valid;            /* [R / K, tmax_p] or NULL */
    void* workspace;
} vtgb_llm_decode_attention_beam_fp8_args;
int vtgb_llm_decode_attention_beam_fp8(const vtgb_llm_decode_attention_beam_fp8_args* a, vtgb_stream_t stream);
typedef struct {
    int32_t dtype;                       /* of logits */
    int32_t R, K, V, N;
    int32_t eos;                         /* or -1 */
    int32_t min_new;
    float penalty;                       /* repetition penalty, > 0 (1: none) */
    const void* logits;                  /* [R, V] */
    const int64_t* seq;                  /* [R, N] generated ids */
    const int64_t* step;                 /* device */
    const float* running;                /* [R / K, K] */
    float* cand_score;                   /* [R / K, 2 K] */
    int32_t* cand_idx;                   /* [R / K, 2 K] */
    void* workspace;
    size_t workspace_bytes;
} vtgb_llm_beam_candidates_args;
int vtgb_llm_beam_candidates(const vtgb_llm_beam_candidates_args* a, vtgb_stream_t stream);

/* ---- Eos-id SETS on the graph decoders (opt-in: eos_sets = "graph"; emit.hip, beam.hip; added at version 601 without a bump).  A request may
 *   name up to VTGB_LLM_EOS_MAX eos ids (Llama-3.1-Instruct's generation config lists three); the list is device int32 [n_eos], duplicates
 *   allowed.  The list lives on the device, so the entries cannot read it: whoever builds it checks 0 <= id < V on the host (ops.eos_list, the
 *   decoders), and the kernels treat an id outside [0, V) as equal to no token -- it blocks nothing, ends nothing and indexes nothing.
 * vtgb_llm_pick_greedy: the greedy emission of one decode step in one launch, one workgroup per row.  logits [B, V] (`dtype`, row stride V;
 *   a row that does not start on 16 bytes -- odd V in bf16 -- is read element by element up to the first boundary, never wide from a misaligned
 *   address).  Per row b, t = the LOWEST index of the maximum (torch.argmax's rule), the listed ids counting as -inf while *step < min_new;
 *   a row with fin[b] set gives t = pad and keeps fin[b]; otherwise fin[b] |= (t in eos_ids).  t goes to tok[b] and out[b, *step] (out
 *   [B, N] int64; *step device int64, clamped to [0, N) before it is used as a column: a wrong step gives a wrong column, never a write
 *   outside out).  The result depends on the row alone, not on B or the row's place.  Logits containing NaN are NOT specified (some index in
 *   [0, V) is written).  VTGB_EINVAL: NULL args / operand (eos_ids may be NULL when n_eos == 0), a dtype other than VTGB_BF16 / VTGB_F32,
 *   non-positive B / V / N, n_eos outside [0, VTGB_LLM_EOS_MAX]; VTGB_EUNSUPPORTED: a misaligned operand (logits 16 bytes; step, tok, out 8;
 *   eos_ids 4) -- on the host, before any launch.
 * vtgb_llm_beam_candidates_eos: vtgb_llm_beam_candidates with the list in place of `eos`: lp[id] = -inf for every listed id while
 *   *step < min_new; everything else, the workspace and the refusals are that entry's (plus n_eos out of range / NULL eos_ids: VTGB_EINVAL, a
 *   misaligned eos_ids: VTGB_EUNSUPPORTED).  With a one-element list the scores and indices equal vtgb_llm_beam_candidates' BIT FOR BIT. */
#define VTGB_LLM_EOS_MAX 8
typedef struct {
    int32_t dtype;                       /* of logits */
    int32_t B, V, N;
    int32_t min_new;
    int32_t n_eos;                       /* 0 .. VTGB_LLM_EOS_MAX */
    int64_t pad;
    const void* logits;                  /* [B, V] */
    const int64_t* step;                 /* device */
    const int32_t* eos_ids;              /* device [n_eos] */
    uint8_t* fin;                        /* [B] bool, read and written */
    int64_t* tok;                        /* [B] */
    int64_t* out;                        /* [B, N], column *step written */
} vtgb_llm_pick_greedy_args;
int vtgb_llm_pick_greedy(const vtgb_llm_pick_greedy_args* a, vtgb_stream_t stream);
typedef struct {
    int32_t dtype;                       /* of logits */
    int32_t R, K, V, N;
    int32_t n_eos;                       /* 0 .. VTGB_LLM_EOS_MAX */
    int32_t min_new;
    float penalty;                       /* repetition penalty, > 0 (1: none) */
    const void* logits;                  /* [R, V] */
    const int64_t* seq;                  /* [R, N] generated ids */
    const int64_t* step;                 /* device */
    const float* running;                /* [R / K, K] */
    const int32_t* eos_ids;              /* device [n_eos] */
    float* cand_score;                   /* [R / K, 2 K] */
    int32_t* cand_idx;                   /* [R / K, 2 K] */
    void* workspace;
    size_t workspace_bytes;
} vtgb_llm_beam_candidates_eos_args;
int vtgb_llm_beam_candidates_eos(const vtgb_llm_beam_candidates_eos_args* a, vtgb_stream_t stream);

/* ---- Repetition penalty on ONE beam (opt-in: penalty_decode = "graph"; emit.hip; added at version 601 without a bump).
 * vtgb_llm_repetition_penalty: HF's RepetitionPenaltyLogitsProcessor on the logits of one decode step.  logits [R, V] (`dtype`, row stride V;
 *   16-byte loads only from 16-byte-aligned addresses, so rows of an odd V are fine), seq [R, N] int64, *step device int64, out [R, V] fp32.
 *   With x = (float)logits[r, i]:  out[r, i] = (x < 0 ? x * penalty : x / penalty)  when i is SEEN in row r, else x -- one correctly rounded fp32
 *   multiply or divide, applied once however often an id repeats.  Index i is seen when it is among seq[r, 0 .. clamp(*step, 0, N)) or equals
 *   start_id (an id that is always seen: T5's decoder start token; -1 for none).  An id outside [0, V) matches no index; entries of seq at or
 *   behind *step are never read.  The result is elementwise: it depends on the row alone, not on R, the grid or the row's place.  logits and
 *   out must not overlap.  VTGB_EINVAL: NULL args / operand, a dtype other than VTGB_BF16 / VTGB_F32, non-positive R / V / N, a penalty that
 *   is not finite and positive; VTGB_EUNSUPPORTED: more than 65535 rows, a misaligned operand (logits, out 16 bytes; seq, step 8) -- on the
 *   host, before any launch. */
typedef struct {
    int32_t dtype;                       /* of logits */
    int32_t R, V, N;
    int32_t start_id;                    /* always seen; -1: none */
    float penalty;                       /* > 0, finite (1: out = (float)logits) */
    const void* logits;                  /* [R, V] */
    const int64_t* seq;                  /* [R, N] ids */
    const int64_t* step;                 /* device */
    float* out;                          /* [R, V] */
} vtgb_llm_repetition_penalty_args;
int vtgb_llm_repetition_penalty(const vtgb_llm_repetition_penalty_args* a, vtgb_stream_t stream);

/* ---- Beam search on the T5 decode step (opt-in: beam_search = "graph+t5"; llm.hip; added at version 601 without a bump).
 * vtgb_llm_attention_rows_beam: vtgb_llm_attention_rows in its decode form -- `pos` given, keys [0, *pos], bias row *pos -- over the caches
 *   k / v of `cache_rows` rows (row stride kv_batch), where K and V of key t of query row r come from cache row
 *   clamp(src_row[r * src_row_stride + t], 0, cache_rows - 1) instead of row r / rows_per_batch (int32 table, stride in elements): the beam
 *   rows keep what they generated in place and re-ordering beams re-orders the table.  One wave per (row, head), key t on lane t % 64, the
 *   rounding points and the order of every sum are vtgb_llm_attention_rows': the output equals that entry's on the gathered cache
 *   (k'[r, :, t] = k[src_row[r, t], :, t]) BIT FOR BIT, in bf16 and in fp32.  Table entries at slots past *pos are not read, neither are K/V
 *   slots past *pos (*pos is clamped to t_pad - 1); a wrong entry at a visible slot gives wrong numbers, never a read outside the caches.
 *   VTGB_EINVAL: NULL src_row, NULL pos, cache_rows < 1, src_row_stride < t_pad, and what vtgb_llm_attention_rows calls so;
 *   VTGB_EUNSUPPORTED: what vtgb_llm_attention_rows refuses, and t_pad > VTGB_LLM_ATTN_ROWS_BEAM_MAX_T (scores and the table rows of four
 *   waves in 64 KiB of LDS) -- on the host, before any launch. */
#define VTGB_LLM_ATTN_ROWS_BEAM_MAX_T 1920
int vtgb_llm_attention_rows_beam(const vtgb_llm_attn_rows_args* a, const int32_t* src_row, int64_t src_row_stride, int32_t cache_rows,
                                 vtgb_stream_t stream);

/* ---- LoRA adapters on the language model's q / k / v projections (lora.hip; added at version 601 without a bump).  An in-place low-rank
 *   update of a projection's output -- videotgb_amd.train.LoraLinear.forward in eval mode (peft 0.4.0 tuners.lora.Linear, unmerged, fp32
 *   adapters), rounding for rounding:
 *     for each segment s, row m, column j in [0, n_s):
 *       t[m, i] = sum_k A_s[i, k] * float(x[m, k])              fp32 accumulation, i < r_s
 *       u       = sum_i B_s[j, i] * t[m, i]                      fp32
 *       d       = rnd(u * scaling_s)                             fp32 product, ONE rounding to `dtype`
 *       y[m, col0_s + j] = rnd(y[m, col0_s + j] + d)
 *   x [rows, K] (row stride ldx) and y [rows, n_cols] (row stride ldy) are `dtype` (VTGB_F32 or VTGB_BF16, both the same); A_s [r_s, K] and
 *   B_s [n_s, r_s] fp32 row-major; 1 <= r_s <= VTGB_LORA_MAX_RANK; 1 .. VTGB_LORA_MAX_SEGMENTS segments, disjoint column ranges of y.
 *   Columns outside every segment keep their bits.  Any rows > 0 (the decode step's <= 128, the prefill's B * P).  The order of every sum
 *   is fixed by (K, r_s): a row's bits do not depend on rows, on its neighbours or on the launch grid.  No atomics, no workspace.
 *   Checked on the host before any launch -- VTGB_EINVAL: NULL args / x / y / A / B, a dtype other than the two, n_seg outside 1 ..
 *   VTGB_LORA_MAX_SEGMENTS, r outside 1 .. VTGB_LORA_MAX_RANK, non-positive rows / K / n_cols / n, ldx < K, ldy < n_cols, a segment past
 *   n_cols, overlapping segments; VTGB_EUNSUPPORTED: K or ldx not a multiple of 4, x not aligned to four elements, y not to one, A not
 *   16-byte or B not 4-byte aligned. */
#define VTGB_LORA_MAX_SEGMENTS 4
#define VTGB_LORA_MAX_RANK 64
typedef struct {
    const float* A;                      /* [r, K]                    */
    const float* B;                      /* [n, r]                    */
    int32_t r, n, col0;                  /* y columns [col0, col0 + n) */
    float scaling;                       /* lora_alpha / r            */
} vtgb_llm_lora_seg;
typedef struct {
    int32_t dtype;                       /* of x and y */
    int32_t K, n_cols, n_seg;
    int64_t rows, ldx, ldy;              /* row strides in elements */
    const void* x;
    void* y;
    vtgb_llm_lora_seg seg[VTGB_LORA_MAX_SEGMENTS];
} vtgb_llm_lora_args;
int vtgb_llm_lora(const vtgb_llm_lora_args* a, vtgb_stream_t stream);

/* The same update on a projection whose K-split reduce was deferred (vtgb_gemm_skinny with defer_reduce and S = n_splits > 1; added at
 *   version 601 without a bump): ONE launch adds the fragments and applies the adapters.  `a->x` is bf16 [rows <= 128, K]; `a->y` is
 *   bf16 [rows, n_cols] and is WRITTEN, NOT READ; `part` holds the fragments workspace[(tile * n_splits + split) * rows + m][128] of the
 *   [rows, n_cols] projection (the layout stated at vtgb_gemm_skinny_args.defer_reduce).  For every column j:
 *       base = rnd_bf16(0 + part[.. split 0 ..] + part[.. split 1 ..] + ...)     in split order: what the reduce launch stores
 *       y    = base                                        outside every segment
 *       y    = rnd(base + rnd(u * scaling))                inside a segment, t and u formed by the sums of vtgb_llm_lora
 *   so the result equals vtgb_gemm_skinny (reduced) followed by vtgb_llm_lora, bit for bit, for every row count, split count, rank and
 *   segment placement; a row's bits do not depend on the other rows.  No atomics, no workspace of its own.  Checked on the host before any
 *   launch: vtgb_llm_lora's checks; VTGB_EINVAL for a dtype other than VTGB_BF16, rows > 128, n_splits outside 2 .. 64, NULL part;
 *   VTGB_EUNSUPPORTED for a part that is not 4-byte aligned (the fragments are read one float per lane). */
int vtgb_llm_lora_parts(const vtgb_llm_lora_args* a, const float* part, int32_t n_splits, vtgb_stream_t stream);

size_t vtgb_pack_skinny_weight_bytes(int32_t N, int32_t K);
int vtgb_pack_skinny_weight(const void* w, int64_t ldw, int32_t N, int32_t K, void* dst, vtgb_stream_t stream);
size_t vtgb_gemm_skinny_workspace_bytes(const vtgb_gemm_skinny_args* a);
int vtgb_gemm_skinny(const vtgb_gemm_skinny_args* a, vtgb_stream_t stream);

/* The same weight stream in fp8 (opt-in: decode_weights = "fp8").  Row n of a weight matrix is stored as OCP e4m3 codes q[n, :] and one power-of-two
 * scale[n] = 2^e, e = the smallest integer with amax[n] * 2^-e <= 448 (0 for a zero row); q = the row times 2^-e rounded to nearest even.  q * scale
 * is exactly a bf16 number, so the entries below compute what vtgb_gemm_skinny computes from the bf16 matrix dq = q * scale, bit for bit:
 *   vtgb_pack_skinny_weight_fp8: quantises a bf16 [N, K] matrix (row amax included) into the kernel's stream -- per (128-row tile, 64-deep k-tile)
 *     one 8 KiB block, row r = 64 bytes, 16-byte slot g = the 8 codes of k 8g .. 8g+7 then the 8 codes of k 32+8g .. 32+8g+7; rows beyond N are
 *     zero codes -- and writes scale_out[N] (fp32).  Half the bytes of vtgb_pack_skinny_weight's form.
 *   vtgb_gemm_skinny_fp8: out = (x . q^T) * scale[n], the scale applied to the fp32 accumulators before a fragment is written; `w` is the
 *     packed stream, w_tiled must be 1 and ldw is ignored.  n_splits, the workspace and defer_reduce are vtgb_gemm_skinny's
 *     (vtgb_gemm_skinny_splits / vtgb_gemm_skinny_workspace_bytes serve both), and so are the consumers of a deferred split.  Only the
 *     16-row blocks of x that hold rows < M are staged and multiplied. */
size_t vtgb_pack_skinny_weight_fp8_bytes(int32_t N, int32_t K);
int vtgb_pack_skinny_weight_fp8(const void* w, int64_t ldw, int32_t N, int32_t K, void* dst, float* scale_out, vtgb_stream_t stream);
int vtgb_gemm_skinny_fp8(const vtgb_gemm_skinny_args* a, const float* w_scale, vtgb_stream_t stream);

/* Either weight stream with a projection bias (LlamaConfig.attention_bias / mlp_bias): out = x . w^T + bias[n], what `F.linear(h, weight, bias)`
 * computes.  w_scale NULL: the bf16 stream, `a` read as vtgb_gemm_skinny reads it; w_scale given: the fp8 stream, as vtgb_gemm_skinny_fp8 reads it
 * (w_tiled must be 1).  bias is fp32 [N], 4-byte aligned, never quantised; entries n >= N of the last 128-row tile are not read.  It is added in
 * fp32 to the accumulators of K split 0 alone, after the fp8 row scale and before the fragment is written -- without a split, before the single
 * rounding to `out` -- so fragment 0 holds acc0 + bias, the other fragments are those of the unbiased call, and every reader that adds the
 * fragments in split order (the second launch, vtgb_llm_rmsnorm_parts, vtgb_llm_rope_cache_parts{,_pos}, vtgb_llm_rope_cache_fp8) rounds
 * ((acc0 + bias) + acc1 + ...) once, unchanged.  n_splits, the workspace and defer_reduce are vtgb_gemm_skinny's.  Errors, before any launch:
 * vtgb_gemm_skinny's for `a`; VTGB_EINVAL for a NULL x / w / out / bias and for w_scale with w_tiled != 1; VTGB_EUNSUPPORTED for a bias that
 * is not 4-byte aligned. */
int vtgb_gemm_skinny_bias(const vtgb_gemm_skinny_args* a, const float* w_scale /* NULL: bf16 stream */, const float* bias /* [N] fp32 */,
                          vtgb_stream_t stream);

/* The same weight stream in MXFP4 (opt-in: decode_weights = "mxfp4"; OCP Microscaling v1.0).  Along K every block of 32 consecutive weights of a
 * row shares one E8M0 scale 2^e: e = floor(log2(amax of the block)) - 2 (0 for an all-zero block), clamped to [-120, 125], stored as the byte
 * e + 127.  An element is w * 2^-e rounded to the nearest e2m1 number (sign; magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 = codes 0 .. 7), ties to the
 * even code, saturating at 6; the sign bit is the weight's own.  code * 2^e is exactly a normal bf16 number, so the entries below compute what
 * vtgb_gemm_skinny computes from the bf16 matrix dq = code * 2^e, bit for bit (the definition, on the host: ops.quantize_mxfp4_rows):
 *   vtgb_pack_skinny_weight_mxfp4: quantises a bf16 [N, K] matrix into the kernel's stream -- per (128-row tile, 64-deep k-tile) one block of
 *     4096 + 256 bytes.  Codes: 16 bytes per (wave v = row / 32, f = row % 16, 8-deep k chunk g = 0 .. 3) at ((v * 16 + f) * 4 + g) * 16, four
 *     dwords [fragment i = (row / 16) % 2][32-deep half h], each the 8 codes of row v * 32 + i * 16 + f at k = 32 h + 8 g .. + 7, two per byte,
 *     the lower k in the low nibble.  Scales: 4 bytes per (v, f) at 4096 + (v * 16 + f) * 4, byte 2 i + h = the E8M0 byte of that row's block h.
 *     Rows beyond N are zero codes under the byte 127.  17 / 32 of the bytes of vtgb_pack_skinny_weight_fp8's form.
 *   vtgb_gemm_skinny_mxfp4: out = x . dq^T (+ bias[n]); the codes are widened to bf16 under their block scale in registers.  `w` is the packed
 *     stream, w_tiled must be 1 and ldw is ignored.  bias NULL, or fp32 [N] as vtgb_gemm_skinny_bias takes it (added to K split 0).  n_splits,
 *     the workspace and defer_reduce are vtgb_gemm_skinny's, and so are the consumers of a deferred split.  Only the 16-row blocks of x that
 *     hold rows < M are staged and multiplied.  Errors, before any launch: vtgb_gemm_skinny's for `a`; VTGB_EINVAL for a NULL x / w / out and
 *     for w_tiled != 1; VTGB_EUNSUPPORTED for a bias that is not 4-byte aligned. */
size_t vtgb_pack_skinny_weight_mxfp4_bytes(int32_t N, int32_t K);
int vtgb_pack_skinny_weight_mxfp4(const void* w, int64_t ldw, int32_t N, int32_t K, void* dst, vtgb_stream_t stream);
int vtgb_gemm_skinny_mxfp4(const vtgb_gemm_skinny_args* a, const float* bias /* NULL: none */, vtgb_stream_t stream);

/* ---- attention for the TRAINABLE stages (config C5, SF flavours): forward + backward, fp32 ---------------------------
 * Replaces, with its autograd, the matmul / softmax / dropout / matmul sequence of InstructBlipQFormerMultiHeadAttention.forward
 * (xinstructblip.py:611-694; BLIP-2 twin xblip2.py) and RopeBertSelfAttention.forward (xropebert.py:243-332; the rotary
 * embedding is applied by the caller): out = dropout(softmax(q k^T * scale + key_mask)) v per (batch, head).  `drop` is the
 * multiplicative dropout mask on the probabilities (0 or 1 / (1 - p); NULL = no dropout): injectable, like the Gumbel noise.
 * q / k / v / out and their gradients are token-major [batch, s, heads * head_dim] with element strides (channel stride 1);
 * dq / dk / dv use the strides of q / k / v, dout those of out.  lse [batch, heads, s_q] is written by the forward and read by
 * the backward; delta is backward scratch of the same size.  head_dim <= 128. */
typedef struct {
    int32_t batch, heads, head_dim, s_q, s_kv;
    const float* q;
    const float* k;
    const float* v;
    int64_t q_tok, kv_tok, q_batch, kv_batch;
    const float* key_mask; /* additive fp32 [batch, s_kv] or NULL */
    const float* drop;     /* [batch, heads, s_q, s_kv] or NULL   */
    float scale;
    float* out;
    int64_t o_tok, o_batch;
    float* lse;
    const float* dout; /* backward only from here */
    float* dq;
    float* dk;
    float* dv;
    float* delta;
} vtgb_attn_train_args;
int vtgb_attn_train_forward(const vtgb_attn_train_args* a, vtgb_stream_t stream);
int vtgb_attn_train_backward(const vtgb_attn_train_args* a, vtgb_stream_t stream);

/* ---- the rest of the training graph (config C5 / the SF flavours) -------------------------------------
 * vtgb_gemm_train: out[M, N] fp32 = op(a) . op(b) (+ bias[N]) for the three GEMMs of a linear layer under autograd
 *   (nn.Linear inside InstructBlipQFormerLayer xinstructblip.py:814-883, RopeBertLayer xropebert.py:450-533 and their backward):
 *     forward  y  = x W^T     a = x  [M, K] k-contiguous, b = W  [N, K] k-contiguous
 *     dgrad    dX = dY W      a = dY [M, N'] k-contiguous (contraction N'), b = W read k-MAJOR (element (k_out, n') at W + n' * ldw + k_out)
 *     wgrad    dW = dY^T X    a = dY read k-major (element (n, m) at dY + m * ld + n), b = X read k-major
 *   x_kmajor = 0: element (row, k) at p + row * ld + k;  1: at p + k * ld + row.  x_dtype: storage, VTGB_F32 or VTGB_BF16 -- operands are
 *   used where they lie (no transposed or converted copy).  compute = VTGB_BF16: operands rounded to bf16 on the way into LDS, MFMA, fp32
 *   accumulation;  VTGB_F32: fp32 FMA with the contraction summed in index order (the exactness mode).  Any M, N, K, ld (16-byte aligned
 *   pointers and ld take the vector path).  Few output tiles under a long contraction (weight gradients): with the workspace given the
 *   contraction is cut into slices, summed afterwards in slice order (deterministic); without it the launch is unsplit.
 * vtgb_col_sum_f32: out[n] = sum_m x[m, n] in a fixed order (bias gradients); `partial` = fp32 workspace [vtgb_col_sum_parts(M), N].
 * vtgb_layernorm_train_forward: sum = x * mask + resid (mask = multiplicative dropout mask or NULL; resid or NULL; `sum` may be NULL when
 *   both are), y = LayerNorm(sum) * gamma + beta, mean / rstd [rows] kept for the backward.  _backward: from dy, sum (= x when there was no
 *   mask and no residual), mean, rstd, gamma -> ds (gradient of sum = of resid), dx = ds * mask (only with a mask; else dx = ds), dgamma,
 *   dbeta [D] -- summed per workgroup in row order into `partial` [vtgb_layernorm_train_partials(rows), 2, D] and then over the partials
 *   in order (deterministic).  D % 4 == 0, D <= 2048.
 * vtgb_gelu_forward / _backward: y = x Phi(x) (erf form, F.gelu's default) and dx = dy (Phi(x) + x phi(x)); n fp32 values. */
typedef struct {
    int32_t compute, M, N, K;
    const void* a;
    int64_t lda;
    int32_t a_dtype, a_kmajor;
    const void* b;
    int64_t ldb;
    int32_t b_dtype, b_kmajor;
    const float* bias; /* [N] or NULL */
    float* out;
    int64_t ldo;
    void* workspace;   /* vtgb_gemm_train_workspace_bytes() bytes, or NULL */
    size_t workspace_bytes;
} vtgb_gemm_train_args;
size_t vtgb_gemm_train_workspace_bytes(const vtgb_gemm_train_args* a);
int vtgb_gemm_train(const vtgb_gemm_train_args* a, vtgb_stream_t stream);
int32_t vtgb_col_sum_parts(int32_t M);
int vtgb_col_sum_f32(const float* x, int64_t ldx, int32_t M, int32_t N, float* out, float* partial, vtgb_stream_t stream);
typedef struct {
    int32_t rows, D;
    float eps;
    const float* x;
    const float* mask;
    const float* resid;
    const float* gamma;
    const float* beta;
    float* sum;
    float* y;
    float* mean;
    float* rstd;
    const float* dy; /* backward only from here */
    float* ds;
    float* dx;
    float* dgamma;
    float* dbeta;
    float* partial;
} vtgb_layernorm_train_args;
int32_t vtgb_layernorm_train_partials(int32_t rows);
int vtgb_layernorm_train_forward(const vtgb_layernorm_train_args* a, vtgb_stream_t stream);
int vtgb_layernorm_train_backward(const vtgb_layernorm_train_args* a, vtgb_stream_t stream);
int vtgb_gelu_forward(const float* x, float* y, int64_t n, vtgb_stream_t stream);
int vtgb_gelu_backward(const float* x, const float* dy, float* dx, int64_t n, vtgb_stream_t stream);

/* ---- the language model's training pass (config C5 under LoRA: videotgb_amd.train.llama_with_grad) ---------------------------
 * Added at version 601 without a version bump (the existing entries are unchanged).  What a LlamaDecoderLayer (transformers
 * modeling_llama.py) runs between its linear layers, forward and backward, fp32 and token-major like the rest of the training graph; every
 * sum in a fixed order, no atomics.  All checks run on the host before any launch.
 * vtgb_rmsnorm_train_forward: LlamaRMSNorm.forward (variance = x.pow(2).mean(-1); x * rsqrt(variance + eps); weight * x) with the residual add
 *   in front of it (LlamaDecoderLayer.forward: hidden_states = residual + hidden_states) folded in: sum = x (+ delta, or NULL; `sum` may be
 *   NULL without a delta), y = gamma * (sum * rstd), rstd [rows] = rsqrt(mean(sum^2) + eps) kept for the backward.
 *   _backward: from dy, sum (= x when there was no delta), rstd, gamma -> ds = rstd * (gamma . dy) - sum * rstd^3 / D * SUM(gamma . dy . sum),
 *   (+ dsum, or NULL: the gradient that reaches `sum` from its other consumers -- the residual stream past this norm -- added in the same
 *   pass; ds may be dsum), the gradient of x and of delta alike.  gamma is frozen under LoRA: there is no dgamma.  VTGB_EINVAL for a NULL operand, a non-positive size
 *   or a buffer that is not 16-byte aligned; VTGB_EUNSUPPORTED unless D % 4 == 0 and D <= 8192.
 * vtgb_rope_train: apply_rotary_pos_emb (q * cos + rotate_half(q) * sin) on the nh query and nkv key heads of x [B, S, (nh + 2 nkv) * hd]
 *   (q heads | k heads | v heads) -> y of the same shape, the v heads copied.  cos / sin: fp32 [S, hd], row = position.  conjugate != 0
 *   applies the transposed rotation: the backward (dx from dy) is the same launch with the flag set.  VTGB_EINVAL for a NULL operand, a
 *   non-positive size, an odd hd or y == x; VTGB_EUNSUPPORTED for hd > 128.
 * vtgb_swiglu_train_forward: LlamaMLP's act_fn(gate_proj(x)) * up_proj(x) on gu [M, 2 I] = [gate | up] -> act [M, I] = silu(gate) * up.
 *   _backward: dgu [M, 2 I] from dact and gu: dgate = dact * up * sig(g) (1 + g (1 - sig(g))), dup = dact * silu(gate).  VTGB_EINVAL for a
 *   NULL operand or a non-positive size.
 * vtgb_attn_train_causal_forward / _backward: eager_attention_forward under the causal mask (softmax(q k^T * scale + causal + key_mask) v
 *   with repeat_kv), on the struct of vtgb_attn_train_forward: key j is visible to query i when j <= i; k / v (and dk / dv) hold kv_heads heads
 *   at the strides kv_tok / kv_batch, query head h reads K/V head h / (heads / kv_heads), and dk / dv of a K/V head are the sums over its
 *   query heads in head order.  The additive key_mask [batch, s_kv] still applies; its entries must be FINITE
 *   (the most negative float, as finfo(float32).min, for a padded key; a literal -inf on the first visible key of a row makes the running maximum
 *   -inf - -inf = NaN -- the non-causal entries share this).  VTGB_EINVAL for NULL args or a NULL operand, a non-positive
 *   size, s_q != s_kv, heads % kv_heads != 0 or a non-NULL drop; VTGB_EUNSUPPORTED for head_dim > 128. */
typedef struct {
    int32_t rows, D;
    float eps;
    const float* x;
    const float* delta; /* or NULL */
    const float* gamma;
    float* sum;         /* required with a delta */
    float* y;
    float* rstd;
    const float* dy; /* backward only from here */
    float* ds;
    const float* dsum; /* or NULL */
} vtgb_rmsnorm_train_args;
int vtgb_rmsnorm_train_forward(const vtgb_rmsnorm_train_args* a, vtgb_stream_t stream);
int vtgb_rmsnorm_train_backward(const vtgb_rmsnorm_train_args* a, vtgb_stream_t stream);
int vtgb_rope_train(const float* x, float* y, const float* cos_t, const float* sin_t, int32_t B, int32_t S, int32_t nh, int32_t nkv, int32_t hd,
                    int32_t conjugate, vtgb_stream_t stream);
int vtgb_swiglu_train_forward(const float* gu, float* act, int32_t M, int32_t I, vtgb_stream_t stream);
int vtgb_swiglu_train_backward(const float* gu, const float* dact, float* dgu, int32_t M, int32_t I, vtgb_stream_t stream);
int vtgb_attn_train_causal_forward(const vtgb_attn_train_args* a, int32_t kv_heads, vtgb_stream_t stream);
int vtgb_attn_train_causal_backward(const vtgb_attn_train_args* a, int32_t kv_heads, vtgb_stream_t stream);

/* ---- gradient exchange (config C5; the one collective of the path) ------------------------------------------------
 * Thin wrapper over RCCL (SURVEY.md 8b "later: vtgb_allreduce_f32", 8e): replaces what Lightning's DDPStrategy does for the reference
 * (configs/trainer/ddp.yaml:4, find_unused_parameters: the sum / mean all-reduce of the trainable gradients once per optimizer
 * step).  One communicator per process (= per GPU); rank 0 creates the id with vtgb_comm_unique_id and the host side hands
 * its VTGB_COMM_ID_BYTES bytes to every rank (any channel: torch.distributed's store, a file, MPI); vtgb_comm_init is
 * collective.  vtgb_allreduce_f32 reduces `count` floats IN PLACE, asynchronously on `stream` (sum, or mean when `average`):
 * the caller allocates its gradients as views of one flat buffer and reduces it in a few large pieces -- xGMI is
 * point-to-point, ring collectives are per-link bound, large messages amortise the ring latency.  RCCL is bound with
 * dlopen at the first call; processes that never call these functions never load it. */
#define VTGB_COMM_ID_BYTES 128
typedef struct vtgb_comm vtgb_comm;
int vtgb_comm_unique_id(void* id_out /* host, VTGB_COMM_ID_BYTES */);
int vtgb_comm_init(vtgb_comm** comm, const void* unique_id /* host */, int32_t rank, int32_t world);
int vtgb_comm_destroy(vtgb_comm* comm);
int vtgb_allreduce_f32(vtgb_comm* comm, float* buf, size_t count, int32_t average, vtgb_stream_t stream);

/* ---- in-library launch timing (used by bench.py for the roofline figure) -------------------
 * While enabled, every GEMM / attention launch of the bf16 path is bracketed by a pair of HIP
 * events recorded on the launch stream (no synchronisation at record time).  vtgb_prof_summary
 * synchronises on the recorded events and returns launch count, summed kernel time and summed
 * algorithmic FLOPs (2*M*N*K per GEMM / convolution of the reference's form, 4*B*H*Sq*Skv*hd per attention) of one kind
 * since the last vtgb_prof_reset. */
#define VTGB_PROF_GEMM 0   /* plain GEMM launches (ViT / Q-Former / TGB / projections)             */
#define VTGB_PROF_ATTN 1
#define VTGB_PROF_CONV 2   /* implicit-GEMM convolution launches of the same kernel (RAFT)          */
void vtgb_prof_enable(int on);
void vtgb_prof_reset(void);
int vtgb_prof_summary(int kind, int64_t* launches, double* ms, double* flops);
/* FLOPs the recorded launches of `kind` actually EXECUTED: smaller than the algorithmic figure of vtgb_prof_summary where
 * loop-invariant work has been hoisted out of a launch (RAFT's GRU convolutions: the `inp` third, see vtgb_raft_update). */
int vtgb_prof_executed_flops(int kind, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* VTGB_H */
