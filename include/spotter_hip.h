/*
 * spotter_hip.h — C-ABI of libspotter_hip.so, the MI355X (gfx950) kernels of
 * the RT-DETRv2 /detect hot path.
 *
 * The reference has no C-ABI: its hot path is the duck-typed HF interface
 * AmenitiesDetector calls (apps/spotter/src/spotter/serve.py:98-117):
 *   processor(images=PIL, return_tensors="pt")           -> sp_preprocess_u8
 *   model(**inputs) (RTDetrV2ForObjectDetection.forward) -> sp_conv2d, sp_maxpool3x3s2,
 *        sp_avgpool2x2_ceil, sp_upsample2x_nearest, sp_layernorm, sp_attention,
 *        sp_msda, sp_rowmax, sp_topk_rows, sp_gather_rows, sp_add_rows, sp_ref_init, sp_box_refine
 *   processor.post_process_object_detection(...)         -> sp_postprocess
 * (HF sources: transformers/models/rt_detr/image_processing_pil_rt_detr.py:
 * 451-462, 508-578; transformers/models/rt_detr_v2/modeling_rt_detr_v2.py:
 * 44-225, 1461-1656, 1797-1881.) spotter_amd/ (Python) implements that
 * interface on top of these entry points; INTEGRATION.md shows the binding.
 *
 * Conventions: plain device pointers (fp32 unless stated), sizes in elements,
 * `stream` is a hipStream_t (NULL = default stream). Every call is async on
 * `stream`, allocates nothing and is safe to capture in a hipGraph (except the
 * first sp_preprocess_u8 per (in, out) size, which uploads its coefficient
 * table). Return: 0 ok, >0 hipError_t, <0 argument error; the message is in
 * sp_last_error() (thread-local). No C++ exception crosses the ABI.
 */
#ifndef SPOTTER_HIP_H
#define SPOTTER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_ABI_VERSION 20

enum sp_act { SP_ACT_NONE = 0, SP_ACT_RELU = 1, SP_ACT_SILU = 2, SP_ACT_GELU = 3 };
/* GEMM operand precision:
 *  SP_PREC_FP32  fp32 MFMA (v_mfma_f32_32x32x2_f32: an exact fp32 fmaf chain);
 *  SP_PREC_BF16  bf16 MFMA with fp32 accumulate (activations rounded RNE to bf16 on load,
 *                weights from Wt_bf16) — the separately reported bf16 variant;
 *  SP_PREC_F32X3 fp32 operands as 3-way bf16 splits x = hi + mid + lo (24 significand bits,
 *                exact for normal fp32), products hi·hi + hi·mid + mid·hi + hi·lo + lo·hi +
 *                mid·mid on bf16 MFMA with fp32 accumulate; the dropped terms sum to <= 2^-24
 *                of |a·b| (one fp32 rounding), so the result is fp32-accurate (every instance checked
 *                against fp64: bit-exact on the six kept products, and inside a derived per-element
 *                bound, in tests/test_gpu_conv_plans.py).
 *                Weights from Wt_bf16 as three planes [3][Cout][K] (plane stride
 *                wt_plane_stride); activations are split while staging;
 *  SP_PREC_F32X2 (ABI v19) the TF32-class tier: fp32 operands as 2-way bf16 splits x = hi + lo + rho with
 *                hi = RNE(x), lo = RNE(x - hi), so |x - hi| <= 2^-8 |x| and |rho| <= 2^-16 |x| (about 16
 *                significand bits kept); products lo·hi + hi·lo + hi·hi (smallest first) on bf16 MFMA with fp32
 *                accumulate. The dropped lo·lo, rho_a·b and a·rho_b sum to <= 3·2^-16 |a·b| (1 + 2^-7) per
 *                product: 256x tighter than SP_PREC_BF16, about 10 bits looser than SP_PREC_F32X3, for half of
 *                SP_PREC_F32X3's MFMAs. Weights from Wt_bf16 as two planes [2][Cout][K] (plane stride
 *                wt_plane_stride); activations and outputs stay fp32 rows; every argument check is
 *                SP_PREC_F32X3's with two planes. */
enum sp_precision { SP_PREC_FP32 = 0, SP_PREC_BF16 = 1, SP_PREC_F32X3 = 2, SP_PREC_F32X2 = 3 };

/* One uint8 RGB HWC image in device memory. */
typedef struct {
  const uint8_t* data;
  int32_t height, width;
  int32_t row_stride; /* bytes between rows (>= 3*width) */
} sp_image_u8;

/*
 * Implicit-GEMM convolution / linear layer on fp32 MFMA (v_mfma_f32_32x32x2f32):
 *   out[m, n] = act( (Σ_k A[m, k] · W[n, k]) · row_scale[m % row_period] · scale[n]
 *                    + shift[n] + res1[m, n] ) + res2[m, n]
 * A is NHWC: pixel (b, y, x) starts at A + ((b*H + y)*W + x)*lda, channels [0, Cin).
 * A2 (optional) is added to A element-wise on load (same indexing, lda2).
 * W is [Cout][KH][KW][Cin] (k contiguous). m = (b*Ho + oy)*Wo + ox.
 * Output row m goes to C + (m / out_rows_per_group)*out_group_stride + (m % out_rows_per_group)*ldc
 * (out_rows_per_group = 0 means M, i.e. plain row-major with ldc).
 * res1/res2 rows use (m*ldr). Linear layers: N=1, H=1, W=rows, KH=KW=1.
 * With a workspace, launches whose tile grid cannot fill the chip split K over the
 * grid's z dimension and combine the partial sums (fixed order) before the epilogue.
 * Corresponds to nn.Conv2d + (Frozen)BatchNorm2d + activation (+ residual)
 * (RN:38-68, RN:225-231, M2:817-835) and nn.Linear (+ activation).
 */
typedef struct {
  const float* A; int64_t lda;
  const float* A2; int64_t lda2;
  int32_t N, H, W, Cin;
  int32_t KH, KW, stride, pad;
  int32_t Ho, Wo;
  const float* Wt; int32_t Cout;
  const float* scale;     /* [Cout] or NULL (1) */
  const float* shift;     /* [Cout] or NULL (0) */
  const float* row_scale; int32_t row_period; /* NULL or [row_period] */
  const float* res1; int64_t ldr1;
  int32_t act;
  const float* res2; int64_t ldr2;
  float* C; int64_t ldc;
  int32_t out_rows_per_group; int64_t out_group_stride;
  float* workspace; int64_t workspace_elems; /* optional fp32 scratch enabling split-K (small M) */
  int32_t precision;         /* sp_precision */
  const uint16_t* Wt_bf16;   /* [Cout][K] bf16 weights (SP_PREC_BF16), [3][Cout][K] (SP_PREC_F32X3),
                              * [2][Cout][K] (SP_PREC_F32X2) */
  int64_t wt_plane_stride;   /* elements between the hi / mid / lo (SP_PREC_F32X3) or hi / lo (SP_PREC_F32X2) planes */
  /* Optional row LayerNorm fused into the epilogue (ABI v8): when ln_gamma is set,
   *   out[m, :] = LayerNorm(acc·row_scale·scale + shift + res1)[m, :] · ln_gamma + ln_beta   (eps ln_eps)
   * over the whole output row — the post-norm "Linear → +residual → LayerNorm" of the AIFI and decoder
   * layers (M2:395-404, 409-423, 426-429, 856-904) and enc_output (M2:1376-1381). Needs the fp32 weights
   * (precision SP_PREC_FP32), Cout a multiple of 128 up to 512, act none, no res2 / grouped rows. */
  const float* ln_gamma;
  const float* ln_beta;
  float ln_eps;
  /* ABI v10: A_bf16 (non-NULL, SP_PREC_BF16) replaces A for sp_conv2d's LDS-DMA tiles: the activations as
   * bf16 rows written by their producer (the bf16 variant's maps), staged as they are instead of rounded per
   * fragment; lda counts elements. */
  const uint16_t* A_bf16;
  /* ABI v10: bf16 activations (the bf16 variant keeps the backbone's maps in bf16). C_bf16 (non-NULL)
   * replaces C: the epilogue result is stored as bf16 (RNE) rows, ldc / out_group_stride in elements.
   * res1_bf16 / res2_bf16 (non-NULL) replace res1 / res2 (bf16 rows, ldr1 / ldr2 in elements). Not with
   * LayerNorm. */
  uint16_t* C_bf16;
  const uint16_t* res1_bf16;
  const uint16_t* res2_bf16;
  /* ABI v13: split-K arrival counters (optional, with a workspace). When set, a split-K launch combines its
   * partial sums inside the GEMM launch: each output tile's last-arriving workgroup adds the tile's partials in
   * fixed split order and applies the epilogue (the same arithmetic as the separate reduce launch, so the
   * result is bit-identical), instead of a second reduce launch. The caller zeroes the array once before first
   * use and gives each concurrently running stream its own; every launch leaves it zero. Launches whose tile
   * grid exceeds splitk_counters_len entries, or tiles without the in-launch form, use the reduce launch. */
  int32_t* splitk_counters; int64_t splitk_counters_len;
} sp_conv_desc;

/*
 * Multi-scale deformable attention v2 core + softmax + sampling-location math
 * (M2:166-225, M2:44-115, method "default"), one decoder layer.
 *   value   [B, S, ld_value] rows, head h channel c at column value_col + h*Dh + c
 *   off_aw  [B*Q, ld_off_aw]: columns [0, H*L*P*2) sampling offsets (h, l, p, xy),
 *           then [H*L*P*2, +H*L*P) attention logits (h, l*P + p)
 *   ref     [B*Q, 4] reference boxes (cx, cy, w, h) in (0, 1)
 *   out     [B*Q, ld_out] with column h*Dh + c
 * Requires B, Q > 0, H*Dh a multiple of 64 <= 1024, 1 <= L <= 4, ld_off_aw >= H*L*P*3, ld_out >= H*Dh,
 * ld_value >= value_col + H*Dh.
 */
typedef struct {
  const float* value; int64_t ld_value; int32_t value_col;
  const float* off_aw; int64_t ld_off_aw;
  const float* ref;
  float* out; int64_t ld_out;
  int32_t B, S, Q, heads, head_dim, levels, points;
  int32_t level_h[4], level_w[4], level_start[4];
  float offset_scale;
  /* ABI v10: value_bf16 (non-NULL) replaces value — the bf16 variant's value projection stored as bf16
   * rows (same ld_value / value_col in elements); sampling and accumulation stay fp32. */
  const uint16_t* value_bf16;
} sp_msda_desc;

int sp_abi_version(void);
const char* sp_last_error(void);
/* ABI v14: what this library was compiled with (no device call). SP_BUILD_FUSED_LN: the fused-LayerNorm
 * GEMM epilogue (sp_conv_desc.ln_gamma; diagnostic builds only); SP_BUILD_BOUNDS: the bounds-check build. */
enum sp_build_flag { SP_BUILD_FUSED_LN = 1, SP_BUILD_BOUNDS = 2 };
int sp_build_flags(void);
/* ABI v14, bounds-check builds (SP_BUILD_BOUNDS): synchronises the device, returns the number of index
 * violations the kernels recorded since the last call (and resets the counts), and writes one line per
 * offending source unit ("file:line hits=… index=… extent=…") into buf. -1 on a product build. */
int64_t sp_bounds_report(char* buf, int64_t cap);
int sp_device_init(int device);
/* Frees the cached resample coefficient tables (the only state kept across
 * calls). Safe to call at any time; the next sp_preprocess_u8 rebuilds what it needs. */
int sp_shutdown(void);

/* RTDetrImageProcessorPil resize (PIL BILINEAR, bit-exact) + rescale 1/255 + HWC→CHW
 * (IPP:451-462, IT:118-122, IT:367). out: [n, 3, out_h, out_w] fp32. */
int sp_preprocess_u8(const sp_image_u8* images, int n, int out_h, int out_w, float* out,
                     void* stream);

int sp_conv2d(const sp_conv_desc* d, void* stream);
/* Test / tuning hook (ABI v7): force the GEMM tile configuration of later sp_conv2d calls made by
 * the CALLING THREAD (-1, the default, = chosen by shape). Nothing on the product path calls it, and
 * no environment variable is read: the production tile choice cannot be changed from outside. */
int sp_set_conv_config(int cfg);
/* The same override for split-K launches only (ABI v11; cfg -1 = the library's choice), a cap on the split-K
 * factor of this thread's later launches (max_splits < 1 = the default, 16) and the fewest 32-deep k-tiles a
 * launch needs to split at all (min_ktiles < 1 = the default, 8): bs1 tuning hooks. */
int sp_set_splitk_config(int cfg, int max_splits, int min_ktiles);
/* Tuning knobs of this thread's later launches (ABI v11; value -1 = the product default), for same-process
 * A/B measurements; nothing on the product path calls it. */
enum sp_tuning_knob {
  SP_TUNE_GLDS_EPILOGUE = 3,  /* split-mode slab epilogue: 4 = outputs stored from the accumulators, else the slab pass */
  SP_TUNE_MSDA_GENERIC = 4,   /* ABI v14: 1 = sp_msda's per-lane kernel where the point-sharing one applies (A/B) */
  SP_TUNE_FOLD = 5,           /* the folded split-K tile (sp_set_plan_batch): 1 = never (the split launch + reduce), 2 = for every
                               * split-K launch of the register-staged 64x64 tile (tests, A/B; bit-identical either way) */
};
int sp_set_tuning(int knob, int value);
/* ABI v18: the kernel instantiation sp_conv2d would launch for this descriptor under the calling thread's
 * overrides (sp_set_conv_config, sp_set_splitk_config, sp_set_tuning): sp_conv2d's argument checks and tile
 * choice without a launch. It touches no device and dereferences no pointer of the descriptor (nullness and
 * alignment only). Returns 0, or < 0 with the sp_last_error text sp_conv2d would give. */
enum sp_conv_family {
  SP_CONV_FP32 = 0,      /* conv_gemm_kernel (fp32 MFMA) */
  SP_CONV_MFMA16 = 1,    /* conv_mfma16_kernel (register-staged, bf16 / split operands) */
  SP_CONV_GLDS = 2,      /* conv_glds_kernel (LDS-DMA) */
  /* 3-6: retired with the conv_pipe / conv_pp / conv_x3s / conv_x3p kernels; not reused */
  SP_CONV_FUSED_LN = 7,  /* diagnostic builds: conv_gemm_kernel with the row-LayerNorm epilogue */
};
typedef struct {
  int32_t family;    /* sp_conv_family */
  int32_t tile;      /* the tile's public id (sp_set_conv_config: 221, 4, 46, ...; never 100+id / 200+id) */
  int32_t planes;    /* operand planes: 0 fp32, 1 bf16, 2 the 2-way split (SP_PREC_F32X2), 3 the 3-way split */
  int32_t generic;   /* 1: generic gather (Cin % 32 != 0 or unaligned operands), 0: the fast operand path */
  int32_t a_bf16;    /* 1: the bf16-A-rows form of the tile */
  int32_t fast_1x1;  /* 1: the LDS-DMA kernels' 1x1 fast path (V = 2) */
  int32_t epilogue;  /* LDS-DMA epilogue variant 1-4 (1: the plain one, and every other family) */
  int32_t splits;    /* split-K factor (1: none) */
  int32_t counters;  /* 1: split-K combined in the launch (arrival counters), 0: the reduce launch */
} sp_conv_plan_info;
int sp_conv_plan(const sp_conv_desc* d, sp_conv_plan_info* out);
/* Batch-invariant planning (additive to ABI v20; a PRODUCT-PATH call, unlike the sp_set_* hooks above, and like them
 * per calling thread and never read from the environment). While set with batch >= 1 and plan_batch >= 1, a launch
 * whose rows are `batch` images is planned as the launch of `plan_batch` images would be: sp_conv2d, sp_conv_plan, the
 * Winograd stages, sp_conv3x3_winograd and sp_winograd_plan choose the kernel family, the tile, the operand form and
 * the split-K factor for M' = M * plan_batch / batch rows (M: the launch's rows, N*Ho*Wo, or the Winograd tile count
 * T) and run that choice on the M rows given. sp_set_plan_batch(0, 0), the initial state, plans from M. Returns 0,
 * or < 0 for any other argument below 1.
 *
 * THE INVARIANT: a row's output bits depend only on the row's operands, the descriptor's per-image fields and
 * plan_batch, never on batch (nor on which slot of the batch the image takes).
 *
 * While it is set (batch >= 1, whether or not batch == plan_batch):
 *  - M % batch != 0 is an argument error;
 *  - the split-K factor is the one M' rows give with this descriptor's workspace_elems; a workspace too short for
 *    that factor on the M rows of the launch (splits * M * ldp elements) is an argument error, never a smaller
 *    factor. Callers size the workspace for splits * M;
 *  - the 1x1 fast path's 32-bit addressing limit (M * lda * 4 < 2^32) is the launch's own: see fast_1x1 below.
 * The plan queries answer under the same setting from the same functions the launches run (the rule of v18 / v20).
 *
 * sp_conv_plan_info under the setting. family, tile, planes, generic, a_bf16 and splits follow M' (generic and
 * a_bf16 never depended on M). The others are addressing or resource limits of the launch at hand and keep
 * following M; their alternatives are bit-identical:
 *  - counters (needs splitk_counters_len >= the launch's tiles and slabs below 2^31 bytes): the in-launch combine
 *    sums the slabs in z order with splitk_reduce_kernel's arithmetic
 *    (tests/test_gpu_kernels.py::test_splitk_in_launch_combine_bit_identical);
 *  - epilogue (variant 4 needs the output rows below 2^31 bytes): only variant 4 against variant 2 depends
 *    on M, and the two store the same values (tests/test_gpu_kernels.py::test_direct_store_epilogue_bit_identical);
 *  - fast_1x1 (needs M * lda * 4 < 2^32): the same MFMA sequence on the same operands, only the address arithmetic
 *    differs (tests/test_gpu_batch_invariant.py::test_fast_1x1_is_bit_identical).
 * Where a split is planned for M' and a grid of M rows would not split, the register-staged 64x64 tile runs it
 * folded: one workgroup per tile walks the k-ranges in turn and adds the partial tiles in z order in registers,
 * bit-identical to the split launch + reduce (tests/test_gpu_batch_invariant.py::test_folded_matches_split_reduce);
 * the plan reports the same splits either way. */
int sp_set_plan_batch(int batch, int plan_batch);

/* 3x3 stride-1 pad-1 convolution by Winograd F(2x2, 3x3) (ABI v9): the same result contract as
 * sp_conv2d on the same descriptor (KH = KW = 3, stride 1, pad 1; act, scale / shift, res1 / res2 as
 * above; no A2, row_scale, grouped rows or LayerNorm; Cin % 32 == 0, Cout % 4 == 0, 16-byte aligned
 * operands), computed as input transform V = B^T d B per 2x2 output tile → 16 batched GEMMs
 * V_ab · U_ab on the split (SP_PREC_F32X3 / SP_PREC_F32X2) or bf16 (SP_PREC_BF16) MFMA kernels → output transform
 * Y = A^T M A + the fused epilogue. 2.25x fewer GEMM multiply-adds than the implicit GEMM; fp32 error
 * on par with the direct fp32 conv. Each stage is tested on its own against fp64 (tests/test_gpu_winograd.py on
 * tests/wino_refs.py: both transforms bit for bit on integers, the component GEMM bit for bit on its kept-product
 * model, the whole path bit for bit on impulses; on N(0,1) / offset / post-relu maps the worst error over the
 * derived bound is 0.49 for either transform, 0.12 / 0.07 / 0.30 for the whole path in x3 / x2 / bf16). wt_wino: the transformed weights U = G g G^T (computed in fp64 on
 * the host, rounded to fp32) as bf16 planes [planes][16][Cout][Cin] (component ab = 4a + b), planes
 * wino_plane_stride elements apart (3 planes for SP_PREC_F32X3, 2 for SP_PREC_F32X2, 1 for SP_PREC_BF16); d->Wt /
 * d->Wt_bf16 are not read. work: fp32 scratch of >= 16 * T * (Cin + Cout) elements,
 * T = N * ceil(H/2) * ceil(W/2). Replaces sp_conv2d for the RepVGG 3x3 (M2:921-923) and other
 * stride-1 3x3 convs (M2:817-835, RN:78-103). */
int sp_conv3x3_winograd(const sp_conv_desc* d, const uint16_t* wt_wino, int64_t wino_plane_stride, float* work,
                        int64_t work_elems, void* stream);
/* The three stages of sp_conv3x3_winograd as separate launches (same arguments and checks; work holds
 * V = work[0 : 16*T*Cin) and M = work[16*T*Cin : 16*T*(Cin+Cout))), so a caller can time the component
 * GEMM apart from the two HBM-bound transforms: input transform A → V; the 16 batched GEMMs V → M;
 * output transform + epilogue M → C. */
int sp_winograd_f23_input(const sp_conv_desc* d, float* work, int64_t work_elems, void* stream);
int sp_winograd_f23_gemm(const sp_conv_desc* d, const uint16_t* wt_wino, int64_t wino_plane_stride, float* work,
                         int64_t work_elems, void* stream);
int sp_winograd_f23_output(const sp_conv_desc* d, const float* work, int64_t work_elems, void* stream);
/* The same three stages for F(4x4, 3x3) (ABI v9): 4x4 output tiles, T = N * ceil(H/4) * ceil(W/4), 36
 * components (component ab = 6a + b), interpolation points (0, -1, 1, 1/2, -2, inf); wt_wino
 * [planes][36][Cout][Cin] (U = G g G^T in fp64 on the host), work >= 36 * T * (Cin + Cout) elements.
 * 1/4 of the direct conv's multiply-adds; fp32 error 3-5x the direct conv's, under 1e-5 of the output
 * scale (tests/test_gpu_kernels.py::test_winograd_is_fp32_accurate). Stage by stage against fp64 in
 * tests/test_gpu_winograd.py (test_input_transform[4], test_output_transform[4], test_component_gemm,
 * test_whole_path, test_grid_stride_loop[in4 / out4]): exact families bit-identical; worst error over the
 * derived bound 0.45 (input), 0.50 (output), 0.21 / 0.04 / 0.22 (whole path, x3 / x2 / bf16). */
int sp_winograd_f43_input(const sp_conv_desc* d, float* work, int64_t work_elems, void* stream);
int sp_winograd_f43_gemm(const sp_conv_desc* d, const uint16_t* wt_wino, int64_t wino_plane_stride, float* work,
                         int64_t work_elems, void* stream);
int sp_winograd_f43_output(const sp_conv_desc* d, const float* work, int64_t work_elems, void* stream);
/* What the Winograd stages would run for a descriptor (ABI v20), under the calling thread's sp_set_conv_config:
 * the stages' argument checks (all but the work / wt_wino pointers, which it does not take) and the component
 * GEMM's tile rule, without a launch or a device call. wm = 2 or 4 (F(2x2) / F(4x4)); wino_plane_stride and
 * work_elems as the stages take them. The stages launch from the same function, so plan and launch cannot
 * disagree. Returns 0, or < 0 with the sp_last_error text the stages would give.
 * The stages refuse (each with its own message) lda < Cin, ldc < Cout, ldr1 / ldr2 < Cout for a given residual,
 * and any of A_bf16 / C_bf16 / res1_bf16 / res2_bf16: they read and write fp32 rows only. */
typedef struct {
  sp_conv_plan_info gemm; /* the batched component GEMM's instance (family SP_CONV_GLDS) */
  int32_t components;     /* 16 or 36: GEMMs in the batch */
  int32_t in_vw;          /* channels per thread of the input transform: 4 for F(2x2); 1 or 2 for F(4x4) */
  int32_t out_vw;         /* ... of the output transform */
  int64_t tiles;          /* T = N * ceil(H/wm) * ceil(W/wm): rows of each component GEMM */
} sp_winograd_plan_info;
int sp_winograd_plan(const sp_conv_desc* d, int wm, int64_t wino_plane_stride, int64_t work_elems,
                     sp_winograd_plan_info* out);

/* The F(4x4) output transform of a 3x3 conv fused into the 1x1 conv that reads it (additive to ABI v20): a
 * bottleneck's conv2 → expand. conv2 and work / work_elems as sp_winograd_f43_output takes them (M already in the
 * workspace: the input and gemm stages have run); expand: the descriptor sp_conv2d would take for the 1x1, with
 * A = conv2's C, lda = its ldc, Cin = its Cout and the same N, H, W (refused otherwise). expand_frag: the expand's
 * hi / mid / lo planes repacked into MFMA fragment order, [Cout/32][K/16][3][64][8] bf16 with element
 * (nb, s, plane, lane, j) = planes[plane][32 nb + lane % 32][16 s + 8 (lane / 32) + j], frag_elems = 3*Cout*K
 * (16-byte aligned); NULL: never fused.
 * The expand is planned like every sp_conv2d launch (the calling thread's overrides, sp_set_plan_batch). Where
 * the plan is an LDS-DMA tile on 32x32x16 MFMAs with three planes and no split-K, K is 128 or 256,
 * Cout % 32 == 0, the expand has no res2 / A2 / row_scale / grouped rows / bf16 rows, conv2 no residual, and the
 * planned rows N*H*W reach min_pixels, ONE persistent kernel computes the expand's output from M, bit-identical to
 * the two launches, and conv2's C rows are NOT written. Otherwise the call is sp_winograd_f43_output(conv2) then the
 * expand's planned launch. sp_winograd_expand_plan says which, without a launch or a device call (has_frag: whether
 * expand_frag would be given); both run the same function. */
typedef struct {
  sp_conv_plan_info expand; /* the expand's own plan (what the unfused path launches) */
  int32_t fused;            /* 1: the fused kernel runs; 0: output transform + the plan above */
  int32_t reserved;
  int64_t tiles;            /* conv2's Winograd tiles T */
  int64_t units;            /* 32-pixel work units of the fused kernel: ceil(T / 2) */
} sp_winograd_expand_plan_info;
int sp_winograd_f43_expand(const sp_conv_desc* conv2, const float* work, int64_t work_elems,
                           const sp_conv_desc* expand, const uint16_t* expand_frag, int64_t frag_elems,
                           int64_t min_pixels, void* stream);
int sp_winograd_expand_plan(const sp_conv_desc* conv2, int64_t work_elems, const sp_conv_desc* expand, int has_frag,
                            int64_t min_pixels, sp_winograd_expand_plan_info* out);

/* NCHW → NHWC (pixel_values layout of the processor contract → conv layout). */
int sp_nchw_to_nhwc(const float* x, float* y, int n, int c, int h, int w, void* stream);
/* Backbone stem conv 1 (RN:71-114: 3x3 stride 2 pad 1, Cin 3, FrozenBN affine M2:748-758, ReLU)
 * read directly from NCHW pixel_values x [n,3,h,w]; wt [cout][27] in (kh, kw, ci) order; y NHWC
 * [n, (h-1)/2+1, (w-1)/2+1, cout]. Replaces sp_nchw_to_nhwc + sp_conv2d for this layer. cout 32 or 64,
 * act 0 (none) or 1 (relu); y 16-byte aligned (8 for the bf16 form). (ABI v6) */
int sp_stem_conv3x3s2_nchw(const float* x, const float* wt, const float* scale, const float* shift, float* y,
                           int n, int h, int w, int cout, int act, void* stream);
/* The same with bf16 output rows (ABI v10: the bf16 variant; fp32 arithmetic, RNE at the store). */
int sp_stem_conv3x3s2_nchw_bf16(const float* x, const float* wt, const float* scale, const float* shift, uint16_t* y,
                                int n, int h, int w, int cout, int act, void* stream);
/* Stem convs 2 and 3 of the bf16 variant (ABI v10): 3x3 stride 1 pad 1, Cin 32 → Cout 32 or 64, dense NHWC
 * bf16 rows in and out, weights w16 bf16 [Cout][3][3][32], FrozenBN (scale, shift) + act (0 none, 1 relu)
 * in fp32, RNE at the store. Direct LDS-halo convolution (RN:78-103). */
int sp_conv3x3_c32_bf16(const uint16_t* x, const uint16_t* w16, const float* scale, const float* shift, uint16_t* y,
                        int n, int h, int w, int cout, int act, void* stream);
/* The same two convs on fp32 rows (ABI v10, the fp32 modes): dense NHWC fp32 rows in and out, weights fp32
 * [Cout][3][3][32] (the packed [Cout][K] form), exact fp32 products with fp32 accumulation
 * (v_mfma_f32_32x32x2_f32). Direct LDS-halo convolution (RN:78-103). */
int sp_conv3x3_c32(const float* x, const float* wt, const float* scale, const float* shift, float* y, int n, int h,
                   int w, int cout, int act, void* stream);
/* The ResNet stage-0 3x3 (Cin 64 → Cout 64, stride 1 pad 1, RN:170-231) on bf16 rows (the bf16 variant):
 * bf16 [64][3][3][64] weights, rows ldx / ldy (both % 8, >= 64, 16-byte aligned)
 * elements apart, fp32 accumulate, BN (+ the optional pre-activation residual res, bf16 rows ldr apart: the
 * basic block's shortcut, RN:170-200) + act in fp32, RNE at the store. */
int sp_conv3x3_c64_bf16(const uint16_t* x, int64_t ldx, const uint16_t* w16, const float* scale, const float* shift,
                        uint16_t* y, int64_t ldy, const uint16_t* res, int64_t ldr, int n, int h, int w, int act,
                        void* stream);
/* The thin 3x3 stride-1 pad-1 convs of the fp32 path on the 3-way bf16 split (ABI v17): fp32 rows in and out,
 * weights as the hi / mid / lo bf16 planes [3][Cout][9*Cin] (k in (tap, channel) order, planes plane_stride
 * elements apart: the SP_PREC_F32X3 operand form), BN (scale, shift) + act (0 none, 1 relu). Direct LDS-halo
 * convolutions, bit-identical to sp_conv2d's SP_PREC_F32X3 path on the same operands.
 * sp_conv3x3_c64_x3: Cin 64 -> Cout 64 (the stage-0 bottleneck 3x3), rows ldx / ldy floats apart (% 4, >= 64).
 * sp_conv3x3_c32_x3: Cin 32 -> Cout 32 or 64 (stem convs 2 / 3), dense rows. */
int sp_conv3x3_c64_x3(const float* x, int64_t ldx, const uint16_t* w_planes, int64_t plane_stride, const float* scale,
                      const float* shift, float* y, int64_t ldy, int n, int h, int w, int act, void* stream);
int sp_conv3x3_c32_x3(const float* x, const uint16_t* w_planes, int64_t plane_stride, const float* scale,
                      const float* shift, float* y, int n, int h, int w, int cout, int act, void* stream);
/* nn.MaxPool2d(3, 2, 1) on NHWC (RN:88). y rows are ldy floats apart (ldy >= c, ldy % 4 == 0), so the
 * result can land in a channel slice of a wider buffer (the fused bottleneck shortcut, ABI v6). x and y 16-byte
 * aligned, c % 4 == 0. NaN inputs are outside the contract: the maxima are fmaxf's, which drops a NaN operand
 * where PyTorch propagates it. */
int sp_maxpool3x3s2(const float* x, float* y, int64_t ldy, int n, int h, int w, int c, void* stream);
/* The same on bf16 rows (ABI v10: the bf16 variant's backbone maps); c % 8 == 0, ldy % 8 == 0. */
int sp_maxpool3x3s2_bf16(const uint16_t* x, uint16_t* y, int64_t ldy, int n, int h, int w, int c, void* stream);
/* nn.AvgPool2d(2, 2, 0, ceil_mode=True) on NHWC (RN:150, RN:202); y rows ldy floats apart as above, x and y
 * 16-byte aligned. fp32 sum in (dy, dx) order divided by the in-map count. */
int sp_avgpool2x2_ceil(const float* x, float* y, int64_t ldy, int n, int h, int w, int c, void* stream);
/* The same on bf16 rows (ABI v10; fp32 sum and divide, RNE to bf16); c % 8 == 0, ldy % 8 == 0. */
int sp_avgpool2x2_ceil_bf16(const uint16_t* x, uint16_t* y, int64_t ldy, int n, int h, int w, int c, void* stream);
/* F.interpolate(scale_factor=2, mode="nearest") into a channel slice (M2:1192). */
int sp_upsample2x_nearest(const float* x, int64_t ldx, float* y, int64_t ldy, int n, int h,
                          int w, int c, void* stream);
/* nn.LayerNorm over the last dim (0 < d <= 1024); rows ldx / ldy >= d floats apart (refused otherwise). d % 4 == 0
 * with ldx, ldy % 4 == 0 and x, y, gamma, beta 16-byte aligned takes the float4 kernels, anything else the scalar
 * one. */
int sp_layernorm(const float* x, int64_t ldx, const float* gamma, const float* beta, float* y,
                 int64_t ldy, int rows, int d, float eps, void* stream);
/* ABI v15. sp_layernorm at d = 256 with the output rounded RNE to bf16 rows: the bf16 variant's encoder head,
 * whose score projection rounds its operand to bf16 anyway (M2:1587-1593). ldx, ldy % 4 == 0 and >= d; x, gamma,
 * beta 16-byte and y 8-byte aligned. */
int sp_layernorm_bf16(const float* x, int64_t ldx, const float* gamma, const float* beta, uint16_t* y, int64_t ldy,
                      int rows, int d, float eps, void* stream);
/* softmax(Q Kᵀ · scale) V per (batch, head); Q/K/V rows [batch*n, ld], head h at col h*dh. dh in {32, 48, 64};
 * every ld % 4 == 0 and >= heads*dh; q, k, v, o 16-byte aligned (float4 loads and stores). Anything else is
 * refused (-1) before a launch. */
int sp_attention(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                 int64_t ldv, float* o, int64_t ldo, int batch, int n, int heads, int dh,
                 float scale, void* stream);
/* The same on bf16 operands (ABI v11, the bf16 variant): Q / K / V rounded to bf16 as staged, scores, softmax and
 * accumulation in fp32; fp32 rows in and out. */
int sp_attention_bf16(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                      int64_t ldv, float* o, int64_t ldo, int batch, int n, int heads, int dh,
                      float scale, void* stream);
int sp_msda(const sp_msda_desc* d, void* stream);
/* Per row: top-k of x[r, 0:n] (values reduced by max over groups of `reduce_c` consecutive
 * columns first when reduce_c > 1; sigmoid applied first when apply_sigmoid), sorted by
 * value descending, ties by lower index (-0.0 ties with +0.0 and is returned as +0.0). vals may be NULL.
 * Requires k <= 512. */
int sp_topk_rows(const float* x, int64_t ldx, int rows, int n, int reduce_c, int apply_sigmoid,
                 int k, float* vals, int32_t* idx, void* stream);
/* out[r] = max_c x[r*ldx + c], c < C: the per-anchor class max in front of query selection
 * (enc_outputs_class.max(-1).values, M2:1599), spread over the chip; sp_topk_rows(reduce_c = 1)
 * then ranks one key per anchor. */
int sp_rowmax(const float* x, int64_t ldx, int64_t rows, int c, float* out, void* stream);
/* ABI v15. out[r] = max_c (a[r, :] · w[c, :] + bias[c]), c < n: the bf16 variant's score head and its per-anchor
 * class max in one pass (M2:1587-1599), equal bit for bit to sp_conv2d (SP_PREC_BF16, bf16 A rows) + sp_rowmax.
 * a: bf16 rows [rows, lda], w: bf16 [n, k] (k contiguous), n <= 96, k = 256, 16-byte aligned. */
int sp_linear_rowmax_bf16(const uint16_t* a, int64_t lda, const uint16_t* w, const float* bias, int rows, int n,
                          int k, float* out, void* stream);
/* dst[b, i, :] = src[b*src_rows + idx[b, i], :] */
int sp_gather_rows(const float* src, int64_t ld_src, int src_rows, const int32_t* idx, int k,
                   int batch, int d, float* dst, int64_t ld_dst, void* stream);
/* ABI v15. y[r, 0:cols] = a[r, :] + b[r, :] in fp32, written as fp32 rows (y) or rounded RNE to bf16 rows
 * (y_bf16; exactly one of the two): the decoder / AIFI attention input h + pos (M2:395-404, M2:409-423),
 * materialised so the q/k and offset projections load it by LDS-DMA instead of adding it in a register-staged
 * loader (sp_conv_desc.A2). cols % 8 == 0, lda / ldb % 4 == 0, ldy % 8 == 0, 16-byte aligned rows. */
int sp_add_rows(const float* a, int64_t lda, const float* b, int64_t ldb, float* y, uint16_t* y_bf16, int64_t ldy,
                int rows, int cols, void* stream);
/* ref[b,i,:] = sigmoid(delta[b,i,:] + anchors[idx[b,i],:]) (M2:1597-1603, M2:616). */
int sp_ref_init(const float* delta, int64_t ld_delta, const float* anchors, const int32_t* idx,
                int batch, int k, float* ref, void* stream);
/* ref = sigmoid(delta + inverse_sigmoid(ref, 1e-5)) (M2:636-639, M2:548-552). */
int sp_box_refine(const float* delta, int64_t ld_delta, float* ref, int rows, void* stream);
/* post_process_object_detection, use_focal_loss=True (IPP:536-576):
 * scores = sigmoid(logits) → top-k over Q*C → label = i % C, query = i / C, box = xyxy(boxes[query])
 * × (w, h, w, h); counts[b] = #(score > threshold) (results are sorted, so the kept ones are a
 * prefix). target_hw: device int32 [B, 2] (h, w). work: device int32 [B*k]. */
int sp_postprocess(const float* logits, const float* boxes, const int32_t* target_hw, int batch,
                   int q, int c, int k, float threshold, float* scores, int64_t* labels,
                   float* boxes_xyxy, int32_t* counts, int32_t* work, void* stream);

/*
 * JPEG decode (ABI v11): the step in front of A1 — serve.py:96-97 `Image.open(BytesIO(...)).convert("RGB")`,
 * which Pillow runs through libjpeg-turbo (ISLOW integer IDCT, fancy upsampling, integer YCbCr→RGB).
 * Split per file kind. Progressive, multi-scan and every other form: the Huffman entropy decode (a serial bit
 * stream) on the host (sp_jpeg_decode_coefs), everything per pixel on the GPU (sp_jpeg_to_rgb). Baseline / extended
 * sequential files with one interleaved scan (what cameras and Pillow's default save write) may instead leave the
 * host after header parsing and one pass that removes the 0xFF00 stuffing: sp_jpeg_entropy_pack builds a scan
 * package, sp_jpeg_entropy_decode turns it into the same coefficient array on the GPU (opt-in, below).
 * Supported: 8-bit baseline / extended / progressive Huffman JPEGs with 1 (gray) or 3
 * (YCbCr, or RGB per the Adobe / component-id rules of libjpeg) components, luma at the maximum sampling
 * factors and chroma at 1x or 2x below it in each direction, restart intervals. Anything else returns
 * SP_JPEG_UNSUPPORTED (the caller keeps the reference's host decode for that image).
 */
#define SP_JPEG_UNSUPPORTED (-10)
typedef struct {
  int32_t width, height;
  int32_t ncomp;            /* 1 or 3 */
  int32_t color;            /* 0 gray, 1 YCbCr, 2 RGB */
  int32_t progressive;
  int32_t max_h, max_v;     /* maximum sampling factors */
  int32_t h[3], v[3];       /* sampling factors per component */
  int32_t bw[3], bh[3];     /* coefficient blocks per row / block rows per component (MCU-padded) */
  int64_t block_off[3];     /* first block of each component in the coefficient array */
  int64_t total_blocks;     /* coefficient array: total_blocks * 64 int16, natural (row-major) order */
  int64_t plane_off[3];     /* byte offset of each component's sample plane (bw*8 x bh*8) in `work` */
  int64_t plane_bytes;      /* bytes of `work` sp_jpeg_to_rgb needs */
  uint16_t quant[3][64];    /* dequantisation tables (natural order), latched at each component's first scan */
} sp_jpeg_layout;
/* Host: parse the JPEG in data[0:len) into *lay; with coefs != NULL (coef_elems >= total_blocks*64) also run
 * the entropy decode (jdhuff.c / jdphuff.c semantics, including progressive refinement scans and restart
 * markers; truncated data decodes as zeros, as libjpeg does) and write the quantised coefficients. No device
 * call: safe without a GPU. */
int sp_jpeg_decode_coefs(const uint8_t* data, int64_t len, sp_jpeg_layout* lay, int16_t* coefs, int64_t coef_elems);
/* Device: coefficients (device copy of the array above) → RGB: dequantise + ISLOW IDCT per 8x8 block into the
 * component planes in `work`, then fancy upsampling + YCbCr→RGB into rgb (uint8 HWC rows rgb_stride bytes
 * apart, the exact pixels Pillow's convert("RGB") produces). status (device int32, zeroed by the caller; may
 * be NULL) is set to 1 when a block leaves the range in which this integer IDCT and libjpeg-turbo's SIMD one
 * agree (only corrupt or crafted coefficient data does): the caller then keeps Pillow's decode (ABI v12). */
int sp_jpeg_to_rgb(const int16_t* coefs, const sp_jpeg_layout* lay, uint8_t* work, int64_t work_bytes, uint8_t* rgb,
                   int64_t rgb_stride, int32_t* status, void* stream);

/*
 * Batched coefficients → RGB (added under ABI v20): sp_jpeg_to_rgb's two passes over up to SP_JPEG_BATCH_MAX
 * images in two launches in all. The images share one coefficient buffer, one `work` buffer and one RGB arena;
 * one table row per image says where its parts lie and which workgroups of each launch are its own. A workgroup
 * never spans two images: it finds its row by a uniform binary search of the first-workgroup column.
 */
#define SP_JPEG_BATCH_MAX 64
#define SP_JPEG_BATCH_IDCT_BLOCKS 32  /* 8x8 blocks per workgroup of the IDCT launch (as sp_jpeg_to_rgb) */
#define SP_JPEG_BATCH_COLOR_PX 1024   /* pixels per workgroup of the colour launch (256 threads x 4 pixels) */
typedef struct {
  sp_jpeg_layout lay;
  int64_t coef_off;        /* first int16 element of the image's coefficients in the shared buffer */
  int64_t work_off;        /* byte offset of its planes in the shared `work`, a multiple of 16 */
  int64_t rgb_off;         /* byte offset of its first RGB row in the arena; the plan gives multiples of 256 */
  int64_t rgb_stride;      /* bytes between its RGB rows, >= 3 * width; the plan gives packed rows */
  int32_t first_wg_idct;   /* its first workgroup in the IDCT launch: exclusive prefix sum of the counts */
  int32_t first_wg_color;  /* the same for the colour launch */
} sp_jpeg_batch_item;
typedef struct {
  int64_t coef_elems;      /* int16 elements of the shared coefficient buffer */
  int64_t work_bytes;      /* bytes of the shared `work` */
  int64_t rgb_bytes;       /* bytes of the RGB arena */
  int64_t wg_idct;         /* workgroups of the IDCT launch: sum of ceil(total_blocks / 32) */
  int64_t wg_color;        /* workgroups of the colour launch: sum of ceil(width * height / 1024) */
} sp_jpeg_batch_totals;
/* Host: lay out n images (their layouts as sp_jpeg_decode_coefs filled them) in the three shared buffers: fills
 * items[i] (a copy of lays[i], the offsets, packed RGB rows, both prefix columns) and *totals. Each layout passes
 * sp_jpeg_to_rgb's consistency checks and must be packed as the parser writes it (blocks and planes of the
 * components in order, inside total_blocks / plane_bytes). Refused with -1 and a message: a NULL pointer, n outside
 * [1, SP_JPEG_BATCH_MAX], an inconsistent layout, more than 2^31 - 1 workgroups in a launch. No device call. */
int sp_jpeg_batch_plan(const sp_jpeg_layout* lays, int n, sp_jpeg_batch_item* items, sp_jpeg_batch_totals* totals);
/* Device: exactly two launches for the whole batch. coefs / work / rgb are the shared device buffers (coefs 2-byte,
 * work 16-byte, rgb 4-byte aligned); items_dev is the device copy of the table (8-byte aligned; it may travel in the
 * same upload as the coefficients), items_host the same bytes on the host, read here only to check the arguments:
 * every layout as sp_jpeg_batch_plan checks it, every range inside its buffer, the ranges of one buffer pairwise
 * disjoint, strides >= 3 * width, both prefix columns and *totals what the layouts give. status: device int32 [n],
 * zeroed by the caller; status[i] is set to 1 when image i leaves the IDCT envelope (see sp_jpeg_to_rgb) and is
 * written by no other image. The arithmetic is sp_jpeg_to_rgb's own device code, so the pixels are the same.
 * Asynchronous on `stream`; allocates nothing, copies nothing; can be captured in a graph. */
int sp_jpeg_batch_to_rgb(const int16_t* coefs, int64_t coef_elems, const sp_jpeg_batch_item* items_dev,
                         const sp_jpeg_batch_item* items_host, int n, const sp_jpeg_batch_totals* totals, uint8_t* work,
                         int64_t work_bytes, uint8_t* rgb, int64_t rgb_bytes, int32_t* status, void* stream);

/*
 * GPU entropy decode of baseline Huffman scans (added under ABI v20; spotter_amd/csrc/jpeg_entropy.hip): the
 * self-synchronising parallel Huffman decode. The scan package is one byte buffer (pinned host memory, then its
 * device copy): [6 Huffman tables: DC / AC per component, the host decoder's lookup form][nseg + 1 restart
 * segment entries {int64 bit offset, int32 first MCU, int32 first subsequence}][the entropy-coded bytes of all
 * segments with the 0xFF00 stuffing and the RSTn markers removed, each segment byte-aligned, zero padded].
 */
#define SP_JPEG_NOT_ELIGIBLE 1 /* not an error: the file keeps the host entropy decode */
#define SP_JPEG_PKG_SMALL 2    /* pkg_cap < scan->pkg_bytes: call again with a buffer of that size */
typedef struct {
  int32_t ncomp, bpm;             /* components; blocks per MCU (<= 10) */
  int32_t mcux, mcuy;             /* MCU grid */
  int32_t restart_interval;       /* MCUs per restart segment, 0: one segment */
  int32_t sub_bits;               /* subsequence size in bits */
  int32_t slot_comp[10];          /* component of each block slot of an MCU, in scan order */
  int32_t slot_v[10], slot_h[10]; /* the slot's block row / column inside its component's part of the MCU */
  int64_t nmcu, nseg, nsub;       /* MCUs, restart segments, subsequences (one thread each) */
  int64_t tab_off, seg_off, stream_off; /* byte offsets inside the package */
  int64_t stream_bits;            /* entropy-coded bits (whole bytes) */
  int64_t stream_bytes;           /* padded bytes of the stream area (a multiple of 16, >= 16 past the data) */
  int64_t pkg_bytes;              /* bytes of the package to upload */
  int64_t work_bytes;             /* device workspace sp_jpeg_entropy_decode needs */
} sp_jpeg_scan;
/* Host: parse data[0:len) with sp_jpeg_decode_coefs's parser and every one of its rejection rules, fill *lay as
 * sp_jpeg_decode_coefs(.., NULL, 0) does (plus the latched quantisation tables once the package is written) and,
 * for an eligible file (SOF0 / SOF1, 8-bit, Huffman, exactly one scan that holds all components, at most 10
 * blocks per MCU, restart markers regular: the expected numbers, only 0xFF fill bytes before them), write the scan
 * package into pkg[0:scan->pkg_bytes). Returns 0, SP_JPEG_NOT_ELIGIBLE (progressive, multi-scan, irregular
 * restarts: *lay is filled, keep the host path), SP_JPEG_PKG_SMALL (scan->pkg_bytes holds the size to bring),
 * SP_JPEG_UNSUPPORTED (as the host decoder), or -1. No device call. */
int sp_jpeg_entropy_pack(const uint8_t* data, int64_t len, sp_jpeg_layout* lay, sp_jpeg_scan* scan, uint8_t* pkg,
                         int64_t pkg_cap);
/* Device: the uploaded package → coefs (device int16 [total_blocks][64], natural order, the array
 * sp_jpeg_decode_coefs writes; coef_elems >= total_blocks * 64). work: scan->work_bytes device bytes, 16-byte
 * aligned as pkg is. Allocates nothing; every kernel runs on `stream`. *status (device int32, zeroed by the caller,
 * may be shared with sp_jpeg_to_rgb) gets reason bits ORed in when the result must be discarded: 2 a subsequence
 * still unsynchronised after the round budget, 4 an invalid code or coefficient index, 8 bits consumed past a
 * segment's end, 16 a block count that is not MCUs x blocks per MCU, 32 a DC prediction outside int32, 64 a
 * segment that does not end at a block boundary (data after its last block). The caller
 * then runs the file through sp_jpeg_decode_coefs, which accepts or refuses it by the host rules. */
int sp_jpeg_entropy_decode(const uint8_t* pkg, const sp_jpeg_scan* scan, const sp_jpeg_layout* lay, uint8_t* work,
                           int64_t work_bytes, int16_t* coefs, int64_t coef_elems, int32_t* status, void* stream);
/* Host: sp_jpeg_entropy_decode's passes in the kernels' order on the CPU, over the same per-subsequence code
 * (csrc/jpeg_entropy_core.h), for tests without a GPU. pkg and coefs are host memory; *status as above;
 * rounds[0] = cross-workgroup launches in which a state still changed, rounds[1] = the most in-workgroup rounds
 * any workgroup ran (rounds may be NULL). */
int sp_jpeg_entropy_emulate(const uint8_t* pkg, const sp_jpeg_scan* scan, const sp_jpeg_layout* lay, int16_t* coefs,
                            int64_t coef_elems, int32_t* status, int32_t* rounds);

/*
 * The same decode over up to SP_JPEG_BATCH_MAX images in one launch chain (added under ABI v20): eight kernel
 * launches whatever n is, after one memset per contiguous run of coefficient ranges (one for a table as
 * sp_jpeg_batch_plan packs it). The images' packages share one buffer, their entropy workspaces another, their
 * coefficients the buffer sp_jpeg_batch_to_rgb reads; one table row per image says where its parts lie and which
 * workgroups of the two launch shapes are its own (a workgroup never spans two images and finds its row by the
 * uniform binary search sp_jpeg_batch_to_rgb uses).
 */
typedef struct {
  sp_jpeg_scan scan;       /* as sp_jpeg_entropy_pack filled it; tab_off / seg_off / stream_off relative to pkg_off */
  int32_t h[3], v[3];      /* the layout fields the block geometry needs (sp_jpeg_layout h, v, bw, bh) */
  int32_t bw[3], bh[3];
  int64_t block_off[3];    /* sp_jpeg_layout block_off */
  int64_t total_blocks;    /* the image's coefficient range is total_blocks * 64 int16 from coef_off */
  int64_t geom[28];        /* the kernels' geometry record (csrc/jpeg_entropy_core.h Geom) derived from the fields
                              above by the plan; the check recomputes it and refuses a row where it differs */
  int64_t pkg_off;        /* byte offset of its package in the shared package buffer, a multiple of 16 */
  int64_t work_off;        /* byte offset of its entropy workspace in the shared one, a multiple of 16 */
  int64_t coef_off;        /* first int16 element of its coefficients (sp_jpeg_batch_item coef_off) */
  int64_t dc_nchunk;       /* chunks of its DC pass (one thread each) */
  int32_t first_wg_sub;    /* its first workgroup in the per-subsequence launches: prefix sum of ceil(nsub / 256) */
  int32_t first_wg_dc;     /* the same for the DC launches: prefix sum of ceil(dc_nchunk / 256) */
} sp_jpeg_entropy_item;
typedef struct {
  int64_t pkg_bytes;       /* bytes of the shared package buffer */
  int64_t work_bytes;      /* bytes of the shared entropy workspace */
  int64_t wg_sub;          /* workgroups of a per-subsequence launch */
  int64_t wg_dc;           /* workgroups of a DC launch */
} sp_jpeg_entropy_totals;
/* Host: lay out n images for sp_jpeg_entropy_batch_decode. scans[i] / lays[i] as sp_jpeg_entropy_pack filled them,
 * batch_items[i].coef_off from sp_jpeg_batch_plan. Refused with -1 and a message: a NULL pointer, n outside
 * [1, SP_JPEG_BATCH_MAX], a scan sp_jpeg_entropy_decode would refuse, a coefficient range (up to the next image's, or
 * as sp_jpeg_batch_plan packs them) that does not hold total_blocks * 64, more than 2^31 - 1 workgroups. No device
 * call. */
int sp_jpeg_entropy_batch_plan(const sp_jpeg_scan* scans, const sp_jpeg_layout* lays,
                               const sp_jpeg_batch_item* batch_items, int n, sp_jpeg_entropy_item* ent_items,
                               sp_jpeg_entropy_totals* ent_totals);
/* Host: the check sp_jpeg_entropy_batch_decode runs on the host copy of the table before it launches anything: every
 * row's scan as sp_jpeg_entropy_decode checks it, the row's geometry fields consistent with the scan, every package /
 * workspace / coefficient range aligned and inside its buffer, the ranges of one buffer pairwise disjoint, both prefix
 * columns and *totals what the rows give. 0, or -1 and a message. No device call. */
int sp_jpeg_entropy_batch_check(const sp_jpeg_entropy_item* items, int n, const sp_jpeg_entropy_totals* totals,
                                int64_t pkg_bytes, int64_t work_bytes, int64_t coef_elems);
/* Device: the launch chain for the whole chunk. pkgs_dev: the packages at their pkg_off (16-byte aligned), items_dev
 * the device copy of the table (8-byte aligned; it may travel behind the packages in the same upload), items_host
 * the same bytes on the host, read only by sp_jpeg_entropy_batch_check. work 16-byte aligned. status: device int32
 * [n], zeroed by the caller: status[i] gets image i's reason bits (as sp_jpeg_entropy_decode's) and nobody else's;
 * it is the array sp_jpeg_batch_to_rgb ORs its envelope flag into afterwards. Asynchronous on `stream`; allocates
 * nothing, copies nothing. */
int sp_jpeg_entropy_batch_decode(const uint8_t* pkgs_dev, int64_t pkg_bytes, const sp_jpeg_entropy_item* items_dev,
                                 const sp_jpeg_entropy_item* items_host, int n, const sp_jpeg_entropy_totals* totals,
                                 uint8_t* work, int64_t work_bytes, int16_t* coefs, int64_t coef_elems,
                                 int32_t* status, void* stream);
/* Host: sp_jpeg_entropy_batch_decode's passes on the CPU, walking the table workgroup by workgroup as the kernels do
 * (the binary search included), over the same per-subsequence code. pkgs, work, coefs, status are host memory. */
int sp_jpeg_entropy_batch_emulate(const uint8_t* pkgs, int64_t pkg_bytes, const sp_jpeg_entropy_item* items, int n,
                                  const sp_jpeg_entropy_totals* totals, uint8_t* work, int64_t work_bytes,
                                  int16_t* coefs, int64_t coef_elems, int32_t* status);

/*
 * JPEG encode (ABI v12): serve.py:139-142 `image.save(buffer, format="JPEG")`, which Pillow runs through
 * libjpeg-turbo with quality 75 (or the caller's), 4:2:0 (or the caller's subsampling), the ISLOW forward DCT,
 * the Annex K Huffman tables and a JFIF header. Split as the hardware wants it: colour conversion,
 * downsampling, FDCT, quantisation and the Huffman coding itself (per-MCU bit counts, a prefix sum, then
 * every MCU writes its bits at its own offset) on the GPU; the header bytes, the 0xFF byte stuffing and the
 * final padding on the host. The bytes equal Pillow's (tests/test_jpeg_enc.py, tests/test_gpu_jpeg.py).
 */
typedef struct {
  int32_t width, height;
  int32_t quality;              /* 1..100 (Pillow's default -1 resolved to libjpeg's 75) */
  int32_t h0, v0;               /* luma sampling factors (1x1, 2x1 or 2x2); chroma is 1x1 */
  int32_t mcux, mcuy, bpm;      /* MCU grid; blocks per MCU = h0*v0 + 2 */
  int32_t wb0, hb0;             /* luma blocks holding image data (the rest of the MCU grid: dummy blocks) */
  int64_t total_blocks;         /* mcux * mcuy * bpm, in scan (MCU-interleaved) order */
  int64_t work_bytes;           /* device workspace sp_jpeg_enc_rgb needs */
  int64_t bits_cap;             /* device bytes of the entropy-coded bit buffer (worst case) */
  uint16_t quant[2][64];        /* natural order, luma / chroma (jcparam.c jpeg_set_quality) */
  uint16_t recip[2][64];        /* jcdctmgr.c compute_reciprocal of quant << 3: reciprocal, correction, shift */
  uint16_t corr[2][64];
  int16_t shift[2][64];
} sp_jpeg_enc_layout;
/* Host: the layout for a width x height RGB image at quality (-1 = 75) and Pillow's subsampling code (-1 or 2:
 * 4:2:0, 1: 4:2:2, 0: 4:4:4). */
int sp_jpeg_enc_plan(int32_t width, int32_t height, int32_t quality, int32_t subsampling, sp_jpeg_enc_layout* lay);
/* Device: RGB pixels (uint8 rows row_stride bytes apart, pixel_bytes 3 (RGB) or 4 (RGBX)) → the entropy-coded
 * segment, unstuffed and unpadded, MSB first, in bits[0 : ceil(*nbits / 8)); *nbits (device int64) is written.
 * work: lay->work_bytes; bits: lay->bits_cap bytes. */
int sp_jpeg_enc_rgb(const uint8_t* rgb, int64_t row_stride, int32_t pixel_bytes, const sp_jpeg_enc_layout* lay,
                    uint8_t* work, int64_t work_bytes, uint8_t* bits, int64_t bits_cap, int64_t* nbits, void* stream);
/* Host: the JPEG file: SOI, JFIF APP0, COM (comment_len > 0), DQT x2, SOF0, DHT x4, SOS, the segment with 0xFF
 * stuffing and 1-bit padding, EOI. out_cap >= sp_jpeg_enc_max_bytes(lay, nbits, comment_len). */
int64_t sp_jpeg_enc_max_bytes(const sp_jpeg_enc_layout* lay, int64_t nbits, int64_t comment_len);
int sp_jpeg_enc_finish(const sp_jpeg_enc_layout* lay, const uint8_t* bits, int64_t nbits, const uint8_t* comment,
                       int64_t comment_len, uint8_t* out, int64_t out_cap, int64_t* out_len);

/*
 * Batched encode (added under ABI v20): sp_jpeg_enc_rgb over up to SP_JPEG_BATCH_MAX images in six kernel launches
 * whatever n is (FDCT, per-MCU bit counts, one scan workgroup per image, the segment offsets, the zeroing, the emit;
 * no memset, no copy). The sources are separate device images; the images' workspaces share one buffer and their
 * entropy-coded segments one packed bit buffer, whose layout the device works out from the bit counts. One table row
 * per image says where its parts lie and which workgroups of the two launch shapes are its own (a workgroup never
 * spans two images and finds its row by the uniform binary search sp_jpeg_batch_to_rgb uses). The kernels read the
 * layout, quantiser tables included, from the row in device memory and run sp_jpeg_enc_rgb's own device code on it.
 */
#define SP_JPEG_ENC_FDCT_MCUS 4   /* MCUs per workgroup of the FDCT launch (one wave each, as sp_jpeg_enc_rgb) */
#define SP_JPEG_ENC_WG_MCUS 256   /* MCUs per workgroup of the bit-count and emit launches (one thread each) */
typedef struct {
  sp_jpeg_enc_layout lay;  /* as sp_jpeg_enc_plan filled it */
  const uint8_t* src;      /* the image's pixels: an absolute device pointer (the sources are separate tensors) */
  int64_t row_stride;      /* bytes between its rows, >= pixel_bytes * width */
  int64_t work_off;        /* byte offset of its workspace (lay.work_bytes, laid out as sp_jpeg_enc_rgb's) in the
                              shared one, a multiple of 256 */
  int32_t pixel_bytes;     /* 3 (RGB) or 4 (RGBX) */
  int32_t first_wg_fdct;   /* its first workgroup in the FDCT launch: exclusive prefix sum of ceil(nmcu / 4) */
  int32_t first_wg_mcu;    /* the same for the per-MCU launches: prefix sum of ceil(nmcu / 256) */
  int32_t reserved;        /* 0 */
} sp_jpeg_enc_batch_item;
typedef struct {
  int64_t work_bytes;      /* bytes of the shared workspace */
  int64_t bits_cap;        /* bytes of the packed bit buffer: sum of the layouts' bits_cap, each rounded up to 16 */
  int64_t wg_fdct;         /* workgroups of the FDCT launch */
  int64_t wg_mcu;          /* workgroups of a per-MCU launch */
} sp_jpeg_enc_batch_totals;
/* Host: lay out n images: fills items[i] (a copy of lays[i], work_off, both prefix columns, reserved = 0; src,
 * row_stride and pixel_bytes are the caller's to fill and are left alone) and *totals. Refused with -1 and a message:
 * a NULL pointer, n outside [1, SP_JPEG_BATCH_MAX], a layout that is not sp_jpeg_enc_plan's, more than 2^31 - 1
 * workgroups in a launch. No device call. */
int sp_jpeg_enc_batch_plan(const sp_jpeg_enc_layout* lays, int n, sp_jpeg_enc_batch_item* items,
                           sp_jpeg_enc_batch_totals* totals);
/* Device: the six launches for the whole chunk. items_dev is the device copy of the table (8-byte aligned; it may
 * travel in the same upload as host pixels), items_host the same bytes on the host, read here only to check the
 * arguments before anything launches: every layout sp_jpeg_enc_plan's, every source non-null with pixel_bytes 3 or 4
 * and row_stride >= pixel_bytes * width, every workspace range 256-byte aligned, inside work and the ranges pairwise
 * disjoint, both prefix columns and *totals what the layouts give, work_bytes and bits_cap at least the totals', work
 * 256-byte, bits 16-byte and result 8-byte aligned. A refused call returns -1 and launches nothing.
 * Output: image i's segment, unstuffed and unpadded, MSB first, exactly the bytes sp_jpeg_enc_rgb writes, in
 * bits[seg_off[i] : seg_off[i] + ceil(nbits[i] / 8)); seg_off is computed on the device, in input order, each a
 * multiple of 16 (image i takes its zeroed words, 4 * (ceil(nbits[i] / 32) + 1) bytes, rounded up to 16; bytes
 * between those words and the next segment are left alone). result: device int64 [2n + 1] = nbits[0..n),
 * seg_off[0..n), the bytes used (the end of the last image's part): one small readback, then one download of
 * exactly the used bytes. Asynchronous on `stream`; allocates nothing, makes no host-visible copy. */
int sp_jpeg_enc_batch_rgb(const sp_jpeg_enc_batch_item* items_dev, const sp_jpeg_enc_batch_item* items_host, int n,
                          const sp_jpeg_enc_batch_totals* totals, uint8_t* work, int64_t work_bytes, uint8_t* bits,
                          int64_t bits_cap, int64_t* result, void* stream);

/*
 * Label drawing (ABI v16): serve.py:119-137 `ImageDraw.Draw(image)`, `draw.rectangle`, `draw.text`, whose Python
 * half (colours, layout, anchors, stroke-then-fill) stays Pillow's and whose pixel half — ImagingDrawRectangle and
 * ImagingFill2 with an "L" mask — runs here on the device image (spotter_amd/draw.py records, this applies).
 * An operation covers the pixel rectangle [x0, x1] x [y0, y1] (inclusive, inside the image):
 *   SP_DRAW_FILL   every pixel = ink;
 *   SP_DRAW_BLEND  per channel out = DIV255(out * (255 - m) + ink_c * m), DIV255(a) = (t = a + 128,
 *                  ((t >> 8) + t) >> 8) (Pillow's BLEND8: one rounding of the sum),
 *                  m = masks[mask_off + (sy + y - y0)*mask_stride + sx + x - x0].
 * Operations composite in list order at every pixel (the blend does not commute).
 */
enum sp_draw_kind { SP_DRAW_FILL = 0, SP_DRAW_BLEND = 1 };
#define SP_DRAW_TILE_W 64 /* the pixel tile one workgroup owns */
#define SP_DRAW_TILE_H 8
typedef struct {
  int32_t kind;             /* sp_draw_kind */
  int32_t x0, y0, x1, y1;   /* inclusive pixel rectangle, 0 <= x0 <= x1 < width, 0 <= y0 <= y1 < height */
  uint32_t ink;             /* r | g << 8 | b << 16 (Pillow's draw_ink for RGB) */
  int64_t mask_off;         /* blend: byte offset of the mask's first row in the mask bytes */
  int32_t mask_stride;      /* blend: bytes between mask rows */
  int32_t sx, sy;           /* blend: the mask sample that falls on pixel (x0, y0) */
  int32_t reserved;
} sp_draw_op;
/* One touched tile: pixels [tx*64, +64) x [ty*8, +8) and its operations refs[first : first + count), ascending. */
typedef struct {
  int32_t tx, ty;
  int32_t first, count;
} sp_draw_tile;
/* The packed table sp_draw_pack writes and sp_draw_rgb reads: this header at byte 0, then the sections at the
 * given byte offsets (each 16-byte aligned): ops (sp_draw_op[n_ops]), tiles (sp_draw_tile[n_tiles], ascending by
 * (ty, tx), their ref ranges back to back), refs (int32[n_refs] operation indices), masks (mask_bytes bytes). */
typedef struct {
  int32_t n_ops, n_tiles, n_refs;
  int32_t height, width;    /* the image the tiles were binned for */
  int32_t reserved;
  int64_t ops_off, tiles_off, refs_off, masks_off, mask_bytes;
  int64_t total_bytes;
} sp_draw_table;
/* Host: bin the operations into the tiles they touch and write the packed table (header, operations, tile
 * bins, mask bytes) into out. *need is the table's size; when out is NULL or out_cap < *need nothing else is
 * written (call again with a larger buffer). No device call: safe without a GPU. */
int sp_draw_pack(const sp_draw_op* ops, int32_t n_ops, const uint8_t* masks, int64_t mask_bytes, int32_t height,
                 int32_t width, void* out, int64_t out_cap, int64_t* need);
/* Device: apply a packed table to rgb (uint8 [height, width, 3] rows row_stride bytes apart) in place, in ONE
 * launch with one workgroup per touched tile; every thread keeps four adjacent pixels in registers and walks its
 * tile's operations in list order. table_host is the table as packed (read here, before the launch, to refuse
 * an operation outside the image, a mask range outside the mask bytes, unordered or overlapping tile ranges: <0,
 * nothing launched); table_dev is its device copy (the caller's one H2D copy, ordered before this call on stream). */
int sp_draw_rgb(uint8_t* rgb, int32_t height, int32_t width, int64_t row_stride, const void* table_host,
                const void* table_dev, int64_t table_bytes, void* stream);

/*
 * Batched label drawing (additive to ABI v20): the packed tables of up to SP_DRAW_BATCH_MAX images, each exactly as
 * sp_draw_pack writes it, sit at 16-byte aligned offsets of one batch buffer (one H2D copy) and are applied by ONE
 * launch whatever n is: one workgroup per touched tile of every image. One table row per image says where its pixels
 * and its table lie and which workgroups are its own; a workgroup never spans two images and finds its row by the
 * uniform binary search sp_jpeg_batch_to_rgb uses, then runs sp_draw_rgb's own device code on that image.
 */
#define SP_DRAW_BATCH_MAX 64 /* = SP_JPEG_BATCH_MAX: a decode / encode chunk is one draw batch */
typedef struct {
  uint8_t* rgb;            /* the image's pixels: an absolute device pointer (the images are separate tensors) */
  int32_t height, width;
  int64_t row_stride;      /* bytes between its rows, >= 3 * width */
  int64_t table_off;       /* byte offset of its packed sp_draw_table in the batch buffer, a multiple of 16 */
  int64_t table_bytes;     /* bytes of that table (>= its header's total_bytes) */
  int32_t n_tiles;         /* its touched tiles = its workgroups, > 0 (the table header's n_tiles) */
  int32_t first_wg;        /* its first workgroup in the launch: exclusive prefix sum of n_tiles */
} sp_draw_batch_item;
/* Host: read the n table headers at tables_host + items[i].table_off and fill items[i].n_tiles and first_wg (the
 * other fields are the caller's and are left alone). Returns the launch's workgroup count (the sum of n_tiles), or
 * -1 with a message: a NULL pointer, n outside [1, SP_DRAW_BATCH_MAX], a table_off that is negative, misaligned or
 * leaves no room for a header in tables_bytes, a table without a touched tile (an image with nothing to draw is
 * left out of the batch), more than 2^31 - 1 workgroups. No device call. */
int64_t sp_draw_batch_plan(sp_draw_batch_item* items, int n, const void* tables_host, int64_t tables_bytes);
/* Device: apply every row's table to its image, in place, in one launch. items_dev / tables_dev are the device
 * copies (the caller's one H2D copy, ordered before this call on stream; items_dev 8-byte, tables_dev 16-byte
 * aligned), items_host / tables_host the same bytes on the host, read here only to check the arguments before
 * anything launches: n in [1, SP_DRAW_BATCH_MAX]; per row every check sp_draw_rgb makes of its image and table;
 * table_off 16-byte aligned, [table_off, +table_bytes) inside tables_bytes and the ranges pairwise disjoint; n_tiles
 * > 0 and the table header's; first_wg the exclusive prefix sum; the rows' pixel byte ranges pairwise disjoint (two
 * rows over the same pixels would composite in no defined order). A refused call returns -1 and launches nothing.
 * Asynchronous on `stream`; allocates nothing, makes no host-visible copy. */
int sp_draw_batch_rgb(const sp_draw_batch_item* items_dev, const sp_draw_batch_item* items_host, int n,
                      const void* tables_host, const void* tables_dev, int64_t tables_bytes, void* stream);

/*
 * Cross-process batching (spotter_amd/shared_batch.py): the replica processes of one GPU hand their images to
 * one engine owner through host shared memory. Additive to ABI v20.
 *
 * sp_host_register pins `bytes` of page-aligned (4096) host memory, e.g. a POSIX shared-memory mapping, and
 * returns in *dev_ptr the address kernels use for it; sp_host_unregister releases it. Refused with a message and
 * a non-zero status, nothing changed: p NULL, dev_ptr NULL, bytes <= 0, p not page aligned, a range that
 * overlaps a registered one, an unregister of memory that is not registered.
 */
int sp_host_register(void* p, int64_t bytes, void** dev_ptr);
int sp_host_unregister(void* p);

/* ONE launch that copies n independent fp32 segments (bit patterns kept: NaN payloads, -0.0). src / dst are
 * device memory or the device pointer of registered host memory, 4-byte aligned; the ranges of one call must
 * not overlap. A segment whose src and dst share their offset from 16-byte alignment moves as 16-byte vectors
 * between a scalar head and tail, any other as 4-byte words. A workgroup copies SP_COPY_BLOCK_ELEMS elements
 * of one segment; which segment a workgroup serves is computed on the host into the kernel's by-value
 * argument, so the call uploads nothing, allocates nothing and can be captured in a graph. elems == 0 segments
 * are skipped. Refused with -1 and nothing launched: d NULL, n outside [1, SP_COPY_MAX_SEGMENTS], elems < 0,
 * a NULL or misaligned pointer with elems > 0, more than 2^31 - 1 workgroups. */
#define SP_COPY_MAX_SEGMENTS 64
#define SP_COPY_BLOCK_ELEMS 4096
typedef struct {
  const float* src;
  float* dst;
  int64_t elems;
} sp_copy_segment;
typedef struct {
  int32_t n;
  int32_t reserved;
  sp_copy_segment seg[SP_COPY_MAX_SEGMENTS];
} sp_copy_segments_desc;
int sp_copy_segments(const sp_copy_segments_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPOTTER_HIP_H */
