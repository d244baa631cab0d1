/*
 * vacnic_hip.h — C-ABI of libvacnic_hip.so: the hand-written gfx950 (CDNA4) kernels behind the
 * VACNIC training step.
 *
 * The reference (tingyu215/VACNIC) is pure Python/PyTorch and has no FFI layer; its "plugin
 * boundary" for this path is the torch.nn operator surface of `src/models` plus three trainer
 * helpers.  Every entry point below cites the reference op sequence it replaces
 * (MFULL = src/models/modeling_mmbart_clip_inside_vis_clipcap_ent_type_final_fix_len_enc_self_face_name_ids_crossattn.py,
 *  TRAIN = train_mmbart_enc_self_face_name_ids_retrieve_crossattn_bart_guide_match.py).
 * The Python binding a maintainer would add is the ctypes stub shown in INTEGRATION.md and
 * shipped as vacnic_amd/_lib.py.
 *
 * Conventions
 *  - plain pointers + sizes, no torch types.  All pointers are DEVICE pointers owned by the caller
 *    (PyTorch-ROCm allocator) and borrowed for the stream lifetime of the call.
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*); no hidden syncs,
 *    no device allocation inside the library.
 *  - return value: 0 = ok, otherwise a vacnic_status; vacnic_last_error_string() has the text.
 *  - bf16 tensors are raw uint16 storage ("bf16"), fp32 tensors "f32"; row strides ("ld*") are in
 *    elements.  bf16 row strides must be multiples of 8 (16-byte rows); a K-contiguous GEMM operand
 *    whose K is not a multiple of 8 must have ld >= round_up(K, 8) with finite padding (zero on one side).
 */
#ifndef VACNIC_HIP_H
#define VACNIC_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  VACNIC_OK = 0,
  VACNIC_BAD_SHAPE = 1,
  VACNIC_BAD_DTYPE = 2,
  VACNIC_MISALIGNED = 3,
  VACNIC_HIP_ERROR = 4,
  VACNIC_UNSUPPORTED = 5
} vacnic_status;

const char* vacnic_last_error_string(void);
int vacnic_version(void);

/* ---- activation / epilogue codes ------------------------------------------------------------ */
enum { VACNIC_ACT_NONE = 0, VACNIC_ACT_GELU = 1, VACNIC_ACT_TANH = 2, VACNIC_ACT_QUICKGELU = 3 };

/*
 * GEMM on the MFMA matrix cores (bf16 in, fp32 accumulate).
 *   out[m][n] = epi( alpha * sum_k X(m,k) * W(n,k) + bias[n] ) (+ residual[m][n])
 * x_kstrided = 0: X stored [M][K] (X(m,k) = x[m*ldx + k]);  1: stored [K][M] (x[k*ldx + m]).
 * w_kstrided = 0: W stored [N][K] (torch nn.Linear weight); 1: stored [K][N].
 *   forward  nn.Linear (MFULL:467-483,738-741 q/k/v/out_proj, fc1/fc2 ...): x_k=0, w_k=0
 *   dgrad    dX = dY . W          : X=dY, W=weight viewed [K_red=N][N_out=K]   -> w_kstrided=1
 *   wgrad    dW = dY^T . X        : both operands reduction-strided            -> 1,1 (out_f32_atomic)
 * epilogue:
 *   act            VACNIC_ACT_* applied after bias.
 *   preact         optional bf16 [M][ldo]: receives the pre-activation (saved for backward).
 *   dact_src       optional bf16 [M][ldo]: if non-null, result is multiplied by act'(dact_src)
 *                  (fused activation backward in the dgrad of the following Linear).
 *   residual       optional bf16 [M][ldo] added after the activation.
 *   out_mode       0: bf16 store, 1: f32 store, 2: f32 atomic accumulate (out += ..; split-K ok)
 *   split_k        >=1; >1 requires out_mode 2 or a workspace.  Without a workspace the K slices meet in fp32 atomics, which
 *                  carry alpha and bias only: an activation, preact, dact_src or residual is then VACNIC_UNSUPPORTED.
 *   alignment      x, w, bias: 16 bytes.  out / preact / dact_src / residual: 16 bytes whenever ldo keeps the rows 16-byte
 *                  aligned (bf16: ldo % 8 == 0, fp32 out: ldo % 4 == 0), a bf16 out 8 bytes when ldo % 4 == 0; any other ldo
 *                  takes element-wise accesses.  Otherwise VACNIC_MISALIGNED.
 *   workspace      optional: with split_k > 1 the K slices meet through an ORDERED FIX-UP instead of fp32 atomics — every slice
 *                  deposits its fp32 partial tile here, the last one to arrive sums them in slice order and runs the epilogue
 *                  once — so any out_mode / activation / residual works with split_k > 1 and the result is bitwise
 *                  reproducible.  Needs vacnic_gemm_workspace_bytes(M, N, split_k) bytes (any contents) and `counters`:
 *                  vacnic_gemm_counters(M, N) uint32 words that are ZERO before the call (they are zero again after it).
 *                  Launches that may run concurrently (different streams) must not share either buffer.
 * With out_mode 0 and 256-row tiles the result is rounded to bf16 once (bias and a plain activation are applied in
 * fp32 first); a saved pre-activation, the fused activation backward and the residual are then applied to that bf16
 * value — the arithmetic of a bf16 Linear followed by a bf16 elementwise op.
 */
typedef struct {
  const void* x; const void* w; const float* bias;
  void* out; void* preact; const void* dact_src; const void* residual;
  float* xsum;                    /* optional f32 [M]: xsum[m] += sum_k X(m,k), not scaled by alpha — the bias gradient
                                     (column sums of dY) fused into the weight-gradient GEMM that stages dY anyway
                                     (replaces the separate reduction autograd runs for nn.Linear.bias, MFULL:449-452).
                                     Implemented for x_kstrided && w_kstrided (the weight-gradient layout) only; any
                                     other layout returns VACNIC_UNSUPPORTED */
  int64_t M, N, K;
  int64_t ldx, ldw, ldo;
  int32_t x_kstrided, w_kstrided;
  int32_t act, out_mode, split_k;
  float alpha;
  int32_t tile_hint;              /* 0 = library picks by problem size (M <= 8 rows: the W-streaming skinny kernel); 8 (skinny) / 64 (64x128, 4-deep ring) / 128 / 256 force a config */
  void* workspace;                /* split-K fix-up (see above); NULL = fp32 atomics */
  int64_t workspace_bytes;
  uint32_t* counters;
  int64_t counters_len;           /* words */
  /* activation dropout fused into the epilogue — nn.functional.dropout(act(fc1 x), p=activation_dropout) of the FFN blocks
     (MFULL:649,660,684,740,874) in the forward GEMM (applied after the activation) and the same mask on the gradient in the
     dgrad GEMM that carries dact_src (applied after act'): drop_p in (0, 1), quantised to 1/256; the mask is the function of
     (drop_seed ^ f(*drop_seed_dev), element index m * N + n) that vacnic_dropout_bf16 evaluates, so nothing is stored.
     Needs out_mode 0, ldo == N and N % 16 == 0.  drop_p = 0: off. */
  float drop_p;
  uint64_t drop_seed;
  const uint64_t* drop_seed_dev;
} vacnic_gemm_args;
int vacnic_gemm_bf16(const vacnic_gemm_args* a, void* stream);
/* sizes of the split-K fix-up buffers for an M x N output (upper bounds over every tile configuration the library may pick) */
int64_t vacnic_gemm_workspace_bytes(int64_t M, int64_t N, int64_t split_k);
int64_t vacnic_gemm_counters(int64_t M, int64_t N);

/*
 * Dispatch plan of vacnic_gemm_bf16: what it WOULD launch for these arguments, decided by the very host code the launch path
 * runs (argument checks included: a call vacnic_gemm_bf16 refuses is refused here with the same status).  Touches no GPU and
 * dereferences no operand pointer.  One launch, or two when a small row remainder is cut off into a launch of its own
 * (launch 1 then covers rows [rows[0], M) with 64-row tiles).  Never with fused activation dropout, whose mask depends on the
 * row index inside the whole output.
 */
enum {
  VACNIC_EPI_SKINNY = 0,            /* the skinny kernel's own epilogue (M <= 8) */
  VACNIC_EPI_DIRECT = 1,            /* accumulator registers -> global (64 / 128-row tiles: bf16 out, bias + activation only) */
  VACNIC_EPI_BF16_TRANSPOSED = 2,   /* 256-row tiles: rounded to bf16 once, transposed through LDS; <= 1 extra operand */
  VACNIC_EPI_F32_STAGED = 3,        /* fp32 C tile staged through LDS, 8 outputs per thread (vector or element-wise) */
  VACNIC_EPI_ATOMIC = 4             /* K slices meet in fp32 atomics: alpha and bias only */
};
typedef struct {
  int32_t nlaunch;                /* 1 or 2 */
  int32_t reserved;
  int64_t rows[2];                /* rows of each launch */
  int32_t tile_hint[2];           /* the kernel that runs: 8 skinny, 64 (64x128), 128 / 261 (128x128), 256 / 258 / 260 / 262 (256x256), 264 (256x128) */
  int32_t k_slices[2];            /* effective K slices: min(split_k, ceil(K / 64)) after rounding a slice up to 64 */
  int32_t fixup[2];               /* 1: the slices meet through the ordered fix-up workspace */
  int32_t epilogue[2];            /* VACNIC_EPI_* */
} vacnic_gemm_plan_out;
int vacnic_gemm_plan(const vacnic_gemm_args* a, vacnic_gemm_plan_out* plan);

/*
 * Single-token decoder step: y = epi( LayerNorm(x + residual) . W^T + bias ), M <= 8 rows (beams x batch), K = d_model <= 1024.
 * The post-LN of one decoder sub-block (MFULL:836,859,880: residual add + LayerNorm, eval mode: no dropout) fused as a prologue
 * into the first projection of the next sub-block (q/k/v, cross-attention q, fc1, lm_head); ln_out (bf16 [M][K], optional)
 * receives the normalised rows — the next sub-block's residual.  Bit-identical to vacnic_add_ln_fwd followed by
 * vacnic_gemm_bf16 (skinny kernel).  x / residual rows are contiguous (stride K); act as in vacnic_gemm_bf16; out_mode 0 bf16, 1 f32.
 */
typedef struct {
  const void* x; const void* residual; const float* gamma; const float* beta; void* ln_out;
  const void* w; const float* bias; void* out;
  int64_t M, N, K, ldw, ldo;
  int32_t act, out_mode;
  float eps;
} vacnic_gemv_ln_args;
int vacnic_gemv_ln_bf16(const vacnic_gemv_ln_args* a, void* stream);

/* Grouped weight gradients — nn.Linear backward w.r.t. weight and bias (autograd of MFULL:449-452 and every other Linear of
 * the path) for SEVERAL layers in one launch:
 *     dw[N, K] += dy[M, N]^T . x[M, K]          dbias[N] += column sums of dy   (dbias may be NULL)
 * dy, x bf16 row-major (rows 16-byte aligned: ld % 8 == 0), dw / dbias fp32, accumulated in place.  No split-K and no atomics
 * on dw: every output element has one writer and a fixed summation order (bitwise reproducible).  Each 1024 x 1024 block of
 * a dw runs with its full reduction on one XCD; jobs of one call should share M (they finish together).  The torch reference
 * runs one cuBLAS GEMM + one reduction per Linear. */
typedef struct {
  const void* dy; const void* x;
  float* dw; float* dbias;
  int64_t M, N, K;
  int64_t lddy, ldx, lddw;
} vacnic_wgrad_job;
int vacnic_wgrad_group(const vacnic_wgrad_job* jobs, int64_t njobs, void* stream);

/*
 * Fused attention core (replaces bmm -> +mask -> softmax -> bmm of BartAttention.forward,
 * MFULL:509-548, and nn.MultiheadAttention inside the CLIP ViT).  head_dim must be 64.
 *   q: [B][Tq][..] bf16, row stride ldq, head h at column offset h*64; likewise k, v (rows Tk).
 *   out: [B][Tq][H*64] bf16 (row stride ldo) — heads merged, ready for out_proj.
 *   key_mask: optional uint8 [B][Tk]; 0 => additive finfo(float32).min exactly as _expand_mask
 *             (MFULL:387-398) does (an all-masked row therefore softmaxes uniformly, like torch).
 *   causal:   1 => key j masked for query i when j > i (MFULL:373-385).
 *   scale:    multiplies q.k (reference multiplies q by head_dim**-0.5, MFULL:471).
 *   lse:      f32 [B][H][Tq] log-sum-exp of the scaled+masked scores (saved for backward); finfo(float32).min for a query whose
 *             keys are all masked (an empty batch row), which vacnic_attn_bwd reads as "softmaxed uniformly".
 *   Tk <= 8192 (VACNIC_UNSUPPORTED beyond: the key bias of a row lives in LDS).
 */
typedef struct {
  const void* q; const void* k; const void* v; void* out; float* lse;
  const uint8_t* key_mask;
  int64_t B, H, Tq, Tk;
  int64_t ldq, ldk, ldv, ldo;
  int64_t bsq, bsk, bsv, bso;     /* batch strides in elements */
  int32_t causal; float scale;
  /* attention-probability dropout, nn.functional.dropout(attn_weights, p=attention_dropout) of MFULL:546 (0.1 in the bart-base / bart-large hub configs):
     p_drop in [0,1) quantised to 1/256; Philox keep bits from (seed ^ f(*seed_dev), batch, head, query, key), regenerated by
     vacnic_attn_bwd from the same seed — the [B*H, Tq, Tk] mask is never stored.  lse stays the undropped log-sum-exp. */
  float p_drop; uint64_t seed; const uint64_t* seed_dev;
} vacnic_attn_fwd_args;
int vacnic_attn_fwd(const vacnic_attn_fwd_args* a, void* stream);

typedef struct {
  const void* q; const void* k; const void* v; const void* out; const void* dout;
  const float* lse; float* delta;            /* delta: f32 [B][H][Tq] scratch: sum_k P[q][k] dP[q][k], formed from the kernels' own P and
                                                dP for Tq <= 128 (Tq <= 64: inside the one backward kernel; 64 < Tq <= 128: by a
                                                sweep of the dQ kernel) and as rowsum(dO*O) above */
  void* dq; void* dk; void* dv;              /* bf16, same layouts/strides as q,k,v */
  const uint8_t* key_mask;
  int64_t B, H, Tq, Tk;
  int64_t ldq, ldk, ldv, ldo;
  int64_t bsq, bsk, bsv, bso;
  int64_t lddq, lddk, lddv, bsdq, bsdk, bsdv;
  int32_t causal; float scale;
  float p_drop; uint64_t seed; const uint64_t* seed_dev;      /* as in the forward call */
} vacnic_attn_bwd_args;
int vacnic_attn_bwd(const vacnic_attn_bwd_args* a, void* stream);

/*
 * Attention probabilities (output_attentions=True): the attn_weights_reshaped of BartAttention.forward, MFULL:509-544 —
 *   out[b][h][i][j] = softmax_j( scale * q[b][i][h*64..] . k[b][j][h*64..] + masks ),  fp32 [B][H][Tq][Tk], contiguous,
 * the softmax BEFORE dropout (MFULL:534 vs :546), in train and eval mode alike.  q / k / key_mask / causal / scale exactly as
 * in vacnic_attn_fwd (the fused k|v|q and k|v buffers are passed as strided views); H*64 must fit both row strides.
 * Masked keys and the causal upper triangle come out as exactly 0.0; a row whose keys are all masked is uniform 1/Tk, as torch
 * gives it for the additive finfo.min mask.  Independent of vacnic_attn_fwd's lse (two sweeps over the keys); every element has
 * one writer and a fixed summation order, so two launches give identical bits.  Tk <= 4096 (VACNIC_UNSUPPORTED beyond: the key
 * bias of a row lives in LDS); one Tq x Tk map must stay below 2 GiB.
 */
typedef struct {
  const void* q; const void* k; float* out;
  const uint8_t* key_mask;
  int64_t B, H, Tq, Tk;
  int64_t ldq, ldk;
  int64_t bsq, bsk;               /* batch strides in elements */
  int32_t causal; float scale;
} vacnic_attn_probs_args;
int vacnic_attn_probs(const vacnic_attn_probs_args* a, void* stream);

/*
 * out = LayerNorm(residual + dropout(x)) * gamma + beta   (post-LN blocks, MFULL:651-653,705-707,
 * 721-723,742-744; nn.LayerNorm eps=1e-5).  x/residual/out bf16 [R][D]; residual may be NULL
 * (plain LN: ViT ln_pre/ln_1/ln_2/ln_post, ner_map_layer_norm).  Dropout is Philox keyed on
 * (seed, row*D+col); p = 0 disables it.  mean/rstd f32 [R] are saved for backward.
 */
typedef struct {
  const void* x; const void* residual; const float* gamma; const float* beta;
  void* out; float* mean; float* rstd;
  int64_t R, D; float eps; float p_drop; uint64_t seed;
  const uint64_t* seed_dev;      /* optional device counter mixed into the seed (fresh masks under hipGraph replay) */
} vacnic_add_ln_fwd_args;
int vacnic_add_ln_fwd(const vacnic_add_ln_fwd_args* a, void* stream);
/* out[i] = x[i] * keep_i / (1 - p) on a flat bf16 array (in place allowed; n % 8 == 0): nn.functional.dropout(act(fc1 x),
 * p=activation_dropout) of the FFN blocks (MFULL:649,660,684,740,874) as a stand-alone pass — the same mask the GEMM epilogues
 * apply when vacnic_gemm_args.drop_p is set: p quantised to 1/256, element i keeps iff byte i % 16 of Philox block i / 16 of
 * (seed ^ f(*seed_dev)) is >= round(256 p).  Backward calls it on the gradient with the same seed; nothing is stored. */
int vacnic_dropout_bf16(const void* x, void* out, int64_t n, float p_drop, uint64_t seed, const uint64_t* seed_dev, void* stream);

/* backward: recomputes h = residual + dropout(x) from the saved INPUTS (x, residual) and the saved
 * mean/rstd; writes dresidual (= d h) and dx (= d h * keep/(1-p)); either may be NULL.  With
 * p_drop = 0 the two are identical, pass one.  dgamma/dbeta are accumulated with f32 atomics. */
typedef struct {
  const void* dout; const void* x; const void* residual; const float* gamma;
  const float* mean; const float* rstd;
  void* dresidual; void* dx; float* dgamma; float* dbeta;
  int64_t R, D; float p_drop; uint64_t seed; const uint64_t* seed_dev;
  float* partials; int64_t partial_rows;   /* optional caller-owned scratch f32 [partial_rows][2][D] (partial_rows >= min(1024,
                                              ceil(R/4))): dgamma/dbeta are then reduced in two stages (per-block column sums,
                                              one small fold) instead of ~1000 same-address atomics per column */
  int32_t defer_fold;                      /* 1 (with partials): leave the fold to the caller — vacnic_ln_partial_fold on a stream of
                                              its choice (the parameter gradients are needed only by AdamW / the reducer, so the fold
                                              need not sit in the backward chain) */
  int32_t partials_any;                    /* 0 (a zero-initialised tail): as before, partials are used from 64 blocks (R >= 253) on and
                                              fewer blocks add with atomics.  1 (the deterministic mode): partials are used for every
                                              R >= 1, so that with defer_fold = 1 the kernel performs no atomic at all; the caller folds
                                              rows = min(1024, ceil(R / 4)) with vacnic_fold_ordered.  Block b of the grid always owns
                                              rows b * 4 + w + k * 4 * rows (wave w, k = 0, 1, ...): a function of R alone */
} vacnic_add_ln_bwd_args;
int vacnic_add_ln_bwd(const vacnic_add_ln_bwd_args* a, void* stream);
/* dgamma[D] += sum over rows of partials[row][0][:], dbeta[D] += ... [row][1][:]  (partials f32 [rows][2][D], as written by
 * vacnic_add_ln_bwd with defer_fold = 1 for rows = min(1024, ceil(R / 4))) */
int vacnic_ln_partial_fold(const float* partials, float* dgamma, float* dbeta, int64_t rows, int64_t D, void* stream);

/*
 * out = dropout(LayerNorm(embed[ids]*scale + pos[t + 2]))  — BartEncoder/BartDecoder prologue,
 * MFULL:1243-1249,1254-1260,1553-1562; BartLearnedPositionalEmbedding offset 2 (MFULL:401-418).
 * ids int64 [B][T]; embed f32 or bf16 master table [V][D] (we read the bf16 shadow); pos bf16.
 */
typedef struct {
  const int64_t* ids; const void* embed; const void* pos; const float* gamma; const float* beta;
  void* out; float* mean; float* rstd;
  int64_t B, T, D, V; int64_t pos_offset; float embed_scale; float eps; float p_drop; uint64_t seed;
  const uint64_t* seed_dev;
} vacnic_embed_ln_fwd_args;
int vacnic_embed_ln_fwd(const vacnic_embed_ln_fwd_args* a, void* stream);

typedef struct {
  const int64_t* ids; const void* embed; const void* pos; const void* dout; const float* gamma;
  const float* mean; const float* rstd;
  float* dembed; float* dpos; float* dgamma; float* dbeta;   /* f32 accumulate (atomics); any may be NULL */
  int64_t B, T, D, V; int64_t pos_offset; float embed_scale;
  int64_t padding_idx;                        /* rows with ids == padding_idx get no embedding grad (nn.Embedding) */
  float p_drop; uint64_t seed; const uint64_t* seed_dev;
} vacnic_embed_ln_bwd_args;
int vacnic_embed_ln_bwd(const vacnic_embed_ln_bwd_args* a, void* stream);

/*
 * Fixed-order sums (the deterministic mode, vacnic_amd.ops.set_deterministic).  Every entry point below is a plain grid without
 * atomics or hand-over between workgroups; every output element has one writer, which reads it, adds and writes it back, so two
 * calls onto the same destination compose when they are ordered by their streams.  All additions are fp32, rounded one by one
 * (no contraction), in the order given here — a function of the shapes alone.
 *
 * vacnic_fold_ordered: dst[c] += sum_b partials[b * ld + c] for c < cols; with dst2 also dst2[c] += sum_b partials[b * ld + cols + c].
 *   Order (4 strands): s_w = +0; for b = w, w + 4, w + 8, ... < NB: s_w += partials[b][c];  t = ((s_0 + s_1) + s_2) + s_3;
 *   dst[c] = dst[c] + t.  NB = 0 launches nothing.  VACNIC_BAD_SHAPE: dst null, cols <= 0, NB < 0, ld shorter than a row.
 */
int vacnic_fold_ordered(const float* partials, int64_t ld, float* dst, float* dst2, int64_t NB, int64_t cols, void* stream);
/* dbias[n] += sum_m dy[m][n] (dy bf16 [M][ldy], ldy % 8 == 0) in two stages through partials f32 [partial_rows][N],
 * partial_rows >= rows = vacnic_bias_grad_ordered_rows(M) = clamp(ceil(M / 64), 1, 256).  Stage 1: row block j owns rows
 * [j * rpb, (j + 1) * rpb), rpb = ceil(M / rows); its strand g (of 4) adds rows j * rpb + g, + 4, ... in ascending order from +0 and
 * partials[j][n] = ((g_0 + g_1) + g_2) + g_3.  Stage 2: vacnic_fold_ordered over the rows blocks. */
int64_t vacnic_bias_grad_ordered_rows(int64_t M);
int vacnic_bias_grad_ordered(const void* dy, float* dbias, int64_t M, int64_t N, int64_t ldy, float* partials, int64_t partial_rows,
                             void* stream);
/* src f32 [R][D] (D % 4 == 0, D <= 2048, 16-byte aligned), ids int64 [R]; either destination may be NULL.
 *   dembed[id][:] = dembed[id][:] + scale * (src[r_0][:] + src[r_1][:] + ...) over the rows r_0 < r_1 < ... with ids[r] != padding_idx
 *     and clamp(ids[r], 0, V - 1) == id (the clamp of vacnic_embed_ln_bwd), added in ascending r starting from src[r_0];
 *   dpos[t + pos_offset][:] = dpos[..][:] + (src[t][:] + src[t + T][:] + src[t + 2T][:] + ...) for t < min(T, R), ascending.
 * The product scale * sum is rounded before it is added (never an fma). */
int vacnic_scatter_ordered(const float* src, const int64_t* ids, float* dembed, float* dpos, int64_t R, int64_t T, int64_t D, int64_t V,
                           int64_t pos_offset, int64_t padding_idx, float scale, void* stream);
/* vacnic_embed_ln_bwd without float atomics: every row's dh goes to dh_rows f32 [B T][D], the dgamma / dbeta sums of block b (rows
 * b * 4 + w + k * 4 * rows) to partials f32 [partial_rows][2][D], partial_rows >= rows = min(1024, ceil(B T / 4)); then
 * vacnic_scatter_ordered(dh_rows -> dembed, dpos) and vacnic_fold_ordered(partials -> dgamma, dbeta) on the same stream. */
int vacnic_embed_ln_bwd_ordered(const vacnic_embed_ln_bwd_args* a, float* dh_rows, float* partials, int64_t partial_rows, void* stream);
/* dst[0] = sum_i src[i] (n >= 0; overwrites).  Order (256 strands): s_t = +0; for i = t, t + 256, ... < n: s_t += src[i];
 * total = +0; for t = 0 .. 255: total += s_t. */
int vacnic_sum_ordered(const float* src, int64_t n, float* dst, void* stream);
/* per-row loss terms of the fused LM head, from what vacnic_lmhead_ce_fwd left behind (row_lse, tl, and with label_smoothing > 0
 * part_sum [R][part_tiles], part_tiles = ceil(V / 256)): row_loss[r] = row_lse[r] - tl[r] (+ eps * (tl[r] - mean_j z_j)), an exact 0
 * where targets[r] == ignore_index.  vacnic_sum_ordered(row_loss, R, loss_sum) is the deterministic loss_sum. */
int vacnic_lmhead_row_loss(const float* row_lse, const float* tl, const int64_t* targets, const float* part_sum, int64_t R, int64_t V,
                           int64_t part_tiles, int64_t ignore_index, float label_smoothing, float* row_loss, void* stream);

/*
 * Cross-entropy over materialised logits (CrossEntropyLoss(ignore_index=pad), TRAIN:287,816).
 * logits bf16 or f32 [R][ldl] (first V columns valid); targets int64 [R].
 * vacnic_ce_fwd writes row_lse [R] (and row_loss if non-NULL) and ACCUMULATES *loss_sum / *count
 * (f32 atomics; caller zeroes them) so that loss = loss_sum / count.
 * vacnic_ce_bwd writes dlogits bf16 [R][ldd] = (softmax - onehot) * valid * grad_scale * (*grad_out) / (*count);
 * columns [V, ldd) are zero-filled.  dlogits may alias bf16 logits when ldd == ldl.
 * label_smoothing = eps in [0, 1) (anything else: VACNIC_BAD_SHAPE), torch's CrossEntropyLoss(label_smoothing=eps):
 *   row_loss = (1 - eps) (lse - z_t) + eps (lse - mean_{j < V} z_j),   dlogits = (softmax - (1 - eps) onehot - eps / V) * ...
 * (kernels of their own; eps == 0, e.g. a zero-initialised struct, launches the plain kernels: same row_lse, count and dlogits bit for
 * bit, loss_sum up to the order of its atomic additions).
 */
typedef struct {
  const void* logits; const int64_t* targets; float* row_lse; float* row_loss; float* loss_sum; float* count;
  void* dlogits; const float* grad_out; float grad_scale;
  int64_t R, V, ldl, ldd; int64_t ignore_index; int32_t logits_f32;
  float label_smoothing;
} vacnic_ce_args;
int vacnic_ce_fwd(const vacnic_ce_args* a, void* stream);
int vacnic_ce_bwd(const vacnic_ce_args* a, void* stream);
/* out4 = {total, txt, secla, colam}; total = ce_sum/count + w_secla*secla + w_colam*colam (TRAIN:363).
 * secla / colam may be NULL (treated as 0). */
int vacnic_combine_losses(const float* ce_sum, const float* count, const float* secla, const float* colam,
                          float w_secla, float w_colam, float* out4, void* stream);

/*
 * CoLaM margin loss (TRAIN:296-307,178-182,820): pool(masked mean over T with the LABEL mask,
 * nan_to_num(nan=1)) -> L2 normalise -> cos_i = <a_i, b_i> -> mean_i max(0, margin - cos_i).
 * hs (student, trainable decoder) and hg (guide) bf16 [B][T][D]; mask uint8 [B][T].
 * fwd writes loss (f32 scalar, overwritten) and saves pooled/normalised rows for bwd.
 */
typedef struct {
  const void* hs; const void* hg; const uint8_t* mask;
  float* loss; float* cos; float* pooled_s; float* pooled_g;   /* cos [B]; pooled_* f32 [B][D] (raw pooled, pre-norm) */
  int64_t B, T, D; float margin;
} vacnic_colam_fwd_args;
int vacnic_colam_fwd(const vacnic_colam_fwd_args* a, void* stream);
typedef struct {
  const float* cos; const float* pooled_s; const float* pooled_g; const uint8_t* mask;
  void* dhs;                                  /* bf16 [B][T][D], overwritten */
  int64_t B, T, D; float margin; const float* grad_out; float grad_scale; /* d loss = grad_scale * (*grad_out) */
} vacnic_colam_bwd_args;
int vacnic_colam_bwd(const vacnic_colam_bwd_args* a, void* stream);

/*
 * SECLA face-name loss (BatchSoftmax, TRAIN:631-660): faces f32/bf16 [B][F][D], names f32 [B][N][D].
 *   M1[i][j][n][f] = <name_{i,n}, face_{j,f}>; L1 = CE_i( sum_n max_f M1 / N , target i )
 *   M2[i][j][f][n] = <face_{i,f}, name_{j,n}>; L2 = CE_i( sum_f max_n M2 / F , target i )
 * loss = L1 + L2.  sim f32 [B][N][B][F] scratch holds <name_{i,n}, face_{j,f}> for bwd.
 */
typedef struct {
  const void* faces; const float* names; float* sim; float* logits1; float* logits2; float* loss;
  int64_t B, F, N, D;
} vacnic_secla_fwd_args;
int vacnic_secla_fwd(const vacnic_secla_fwd_args* a, void* stream);
typedef struct {
  const void* faces; const float* names; const float* sim; const float* logits1; const float* logits2;
  void* dfaces;                               /* bf16 [B][F][D], overwritten */
  float* wsim;                                /* f32 [B][N][B][F] scratch: d loss / d sim */
  int64_t B, F, N, D; const float* grad_out; float grad_scale;
} vacnic_secla_bwd_args;
int vacnic_secla_bwd(const vacnic_secla_bwd_args* a, void* stream);

/* Per-name mean of LN(embed_ner(ids)*scale + pos) — get_embedding_ner, TRAIN:112-133 (unmasked
 * mean over the Ln tokens, pads included).  ids int64 [B][Nn][Ln] -> out f32 [B][Nn][D]. */
typedef struct {
  const int64_t* ids; const void* embed; const void* pos; const float* gamma; const float* beta;
  float* out; int64_t B, Nn, Ln, D, V; int64_t pos_offset; float embed_scale; float eps;
} vacnic_name_embed_args;
int vacnic_name_embed_mean(const vacnic_name_embed_args* a, void* stream);

/*
 * Fused AdamW over one flat fp32 arena (torch.optim.AdamW semantics, TRAIN:91):
 *   p *= (1 - lr*wd); m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 *   p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * lr, step are read from device memory (graph-capture safe): hyper = {lr, step(as float)}.
 * Also refreshes the bf16 shadow and zeroes the gradient.  grad_scale multiplies g first
 * (1/world_size for DDP averaging).  clip_coef (may be NULL): device pointer to the clip_grad_norm_
 * coefficient written by vacnic_grad_clip_coef; it multiplies g after grad_scale.
 * skip (may be NULL = never): device pointer to the STEP WORD, an int64 that this entry point, vacnic_adamw_groups, vacnic_adamw_ema
 * and vacnic_param_stats read and that vacnic_grad_guard (its state[0]) or vacnic_lr_step_accum (its accum[0]) writes:
 *   0  apply the step
 *   1  dropped by the guard: the kernel writes no p, m, v and no shadow (no weight decay either) and only zeroes g when zero_grad
 *   2  hold (a micro-batch of an accumulation group that is not its last): the kernel returns before anything is read or written —
 *      p, m, v, the shadow, ema AND g stay as they are, whatever zero_grad says
 */
typedef struct {
  float* p; float* g; float* m; float* v; void* p_bf16; const float* hyper;
  int64_t n; float beta1, beta2, eps, weight_decay, grad_scale; int32_t zero_grad;
  const float* clip_coef;
  const int64_t* skip;
} vacnic_adamw_args;
int vacnic_adamw(const vacnic_adamw_args* a, void* stream);
/* torch.nn.utils.clip_grad_norm_(model.parameters(), clip_norm) (TRAIN:365-366) over the flat gradient arena,
 * without a host sync: out[0] <- min(1, max_norm / (||grad_scale*g||_2 + 1e-6)), out[1] <- that norm.
 * partials: device scratch of >= 1024 floats.  Deterministic (fixed grid, no float atomics).  The gradient is not
 * rewritten; pass `out` as vacnic_adamw_args.clip_coef and the scaling happens where AdamW reads g. */
int vacnic_grad_clip_coef(const float* g, int64_t n, float grad_scale, float max_norm, float* partials,
                          float* out, void* stream);
/*
 * Parameter groups (torch.optim.AdamW(param_groups)): every arena element belongs to one SEGMENT, a contiguous element
 * range with its own learning-rate multiple, weight decay and frozen flag.  The table is built once on the host
 * (vacnic_amd.arena.group_table) and lives in device memory owned by the optimizer:
 *   seg_start  int64 [nseg + 1]   ascending ABSOLUTE arena offsets, seg_start[0] = 0, seg_start[nseg] = arena size
 *   seg        [nseg]             values of segment s = [seg_start[s], seg_start[s + 1])
 *   first_seg  int32 [nblocks]    the segment that holds arena element 1024 * b: where a thread's forward walk starts
 * A boundary may fall on any element; a 4-wide vector that straddles one is updated element by element.  The walk is clamped
 * at nseg - 1 and the block index at nblocks - 1, so a malformed table gives wrong values, never an access outside it.
 *   not frozen: the vacnic_adamw update with lr = hyper[0] * lr_scale and the segment's weight_decay (same arithmetic order)
 *   frozen:     p, m, v and the bf16 shadow are not written; g is still zeroed when zero_grad (backward still accumulates)
 * p, g, m, v, p_bf16 may point INTO the arena (a DDP bucket): elem_base is the arena offset of p[0].
 */
typedef struct { float lr_scale, weight_decay; int32_t frozen; int32_t reserved; } vacnic_adamw_seg;
typedef struct {
  float* p; float* g; float* m; float* v; void* p_bf16; const float* hyper;
  int64_t n; float beta1, beta2, eps, grad_scale; int32_t zero_grad;
  const float* clip_coef;
  const int64_t* seg_start; const vacnic_adamw_seg* seg; const int32_t* first_seg;
  int64_t nseg, nblocks, elem_base;
  const int64_t* skip;                 /* as vacnic_adamw_args.skip */
} vacnic_adamw_groups_args;
int vacnic_adamw_groups(const vacnic_adamw_groups_args* a, void* stream);
/*
 * AdamW with an exponential moving average (EMA) of the weights kept in the same pass.  Null table pointers: the vacnic_adamw
 * update with `weight_decay`; a table: the vacnic_adamw_groups update (weight_decay is then unused).  p, m, v, the shadow and the
 * zeroed g are bitwise what those two entry points write for the same inputs.  Every element that is updated also gets
 *   d = ema_warmup ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay        t = hyper[1], Adam's step count
 *   ema = fma(d, ema, (1 - d) * p_new)
 * (the torch_ema / timm warm-up; a step dropped by vacnic_grad_guard does not advance t).  Elements that are not updated — frozen
 * segments, and every element when *skip != 0 — leave ema unwritten.  ema is laid out parallel to p: it may point into the
 * arena's EMA buffer (a DDP bucket) like p, g, m, v, with elem_base the arena offset of p[0].  ema_decay lies in (0, 1).
 */
typedef struct {
  float* p; float* g; float* m; float* v; void* p_bf16; const float* hyper;
  int64_t n; float beta1, beta2, eps, grad_scale; int32_t zero_grad;
  const float* clip_coef;
  const int64_t* seg_start; const vacnic_adamw_seg* seg; const int32_t* first_seg;
  int64_t nseg, nblocks, elem_base;
  const int64_t* skip;
  float weight_decay;
  float* ema; float ema_decay; int32_t ema_warmup;
} vacnic_adamw_ema_args;
int vacnic_adamw_ema(const vacnic_adamw_ema_args* a, void* stream);
/* Exchange the CONTENTS of p and ema (n fp32 each, n a multiple of 4; addresses stay, so plans, graphs and parameter views hold)
 * and write p_bf16 = bf16(new p), rounded as vacnic_cast_f32_bf16 rounds (p_bf16 may be NULL).  Two calls restore all three. */
int vacnic_ema_swap(float* p, float* ema, void* p_bf16, int64_t n, void* stream);
/* vacnic_grad_clip_coef over the non-frozen elements only (clip_grad_norm_ sees no gradient for a parameter left out of the
 * optimizer): same fixed grid, per-thread order and reduction tree, so with no frozen segment the result is bitwise that of
 * vacnic_grad_clip_coef.  Null table pointers: ungrouped, vacnic_grad_clip_coef itself (only elem_base counts).
 * hold (may be NULL = never, as in a zero-initialised tail): device pointer to vacnic_lr_step_accum's accum.  When *hold == 2 both
 * passes leave at once: the arena is not read and `out` keeps what it held. */
typedef struct {
  const float* g; int64_t n; float grad_scale, max_norm; float* partials; float* out;
  const int64_t* seg_start; const vacnic_adamw_seg* seg; const int32_t* first_seg;
  int64_t nseg, nblocks, elem_base;
  const int64_t* hold;
} vacnic_grad_clip_groups_args;
int vacnic_grad_clip_coef_groups(const vacnic_grad_clip_groups_args* a, void* stream);
/*
 * Non-finite gradient guard, decided on the device (no host sync; recordable in a launch plan).  Call it between vacnic_lr_step
 * and vacnic_adamw[_groups], and pass `state` as their `skip`.  Two passes, as vacnic_grad_clip_coef[_groups] (null table
 * pointers: ungrouped; otherwise frozen segments are left out):
 *   pass 1  the same fixed grid, per-thread order and reduction tree: partials[1024] are bitwise those of the clip-norm pass;
 *           first_idx[1024] (int64) gets, per block, the smallest ABSOLUTE arena element index (elem_base + offset in g) whose
 *           scaled gradient x = g * grad_scale has a non-finite square (NaN, +-Inf, or |x| > ~1.8e19), INT64_MAX if none
 *   pass 2  skip <=> the fp32 sum of squares is not finite.  Squares cannot cancel, so that is exactly: some element's square is
 *           non-finite, or the fp32 sum overflowed although every square is finite (||g|| > ~1.8e19) — then no single element is
 *           to blame and the index reported is -1.
 *   out    float[2]  {min(1, max_norm / (norm + 1e-6)), norm} — for a finite gradient bitwise what vacnic_grad_clip_coef[_groups]
 *                    writes; max_norm <= 0 means no clipping: coefficient 1
 *   state  int64[4]  [0] skip flag of this step   [1] steps skipped so far   [2] current run of consecutive skips (a finite
 *                    step resets it)   [3] first non-finite element index of the most recent skipped step (-1: none yet, or
 *                    only the sum overflowed).  The caller initialises it to {0, 0, 0, -1}.
 *   hyper            on a skip hyper[1] -= 1, undoing vacnic_lr_step's increment: a dropped step advances neither Adam's t nor
 *                    the schedule position (the next vacnic_lr_step recomputes hyper[0] from the same k).  The dropout counter
 *                    that vacnic_lr_step advanced stays advanced: the retried position draws fresh masks.
 *   hold             (may be NULL = never, as in a zero-initialised tail) device pointer to vacnic_lr_step_accum's accum.  When
 *                    *hold == 2 pass 1 leaves at once without reading the arena and pass 2 writes state[0] = 2 and nothing else:
 *                    nothing is counted, hyper and `out` stay.  On the group's last micro-batch (*hold == 0) the guard judges the
 *                    accumulated gradient as above; a dropped group takes back the increment vacnic_lr_step_accum made.
 */
typedef struct {
  const float* g; int64_t n; float grad_scale, max_norm; float* partials; int64_t* first_idx; float* out; int64_t* state;
  float* hyper;
  const int64_t* seg_start; const vacnic_adamw_seg* seg; const int32_t* first_seg;
  int64_t nseg, nblocks, elem_base;
  const int64_t* hold;
} vacnic_grad_guard_args;
int vacnic_grad_guard(const vacnic_grad_guard_args* a, void* stream);
/*
 * Per-parameter gradient and weight statistics (what wandb.watch(model), TRAIN:456, reports per parameter), computed on the device
 * and GATED on the device: no host sync, no allocation, recordable in a launch plan and capturable in a hipGraph like
 * vacnic_grad_guard.  Call it after vacnic_lr_step (and after vacnic_grad_guard when there is one) and BEFORE vacnic_adamw*, which
 * zeroes g.
 * Layout tables, built once on the host (vacnic_amd.arena.stats_table) and resident in device memory:
 *   a SLOT is the element range of one parameter in the arena; slots ascend, are disjoint, and may start and end on ANY element
 *   (members of a fused group are adjacent and unaligned).  Alignment gaps, padded rows and the arena's tail lie in no slot and
 *   are never read into a result.  Every slot is cut into UNITS of at most 4096 elements; a unit never crosses a slot.
 *   unit_off   int64 [nunit]       arena offset of the unit's first element, ascending
 *   unit_len   int32 [nunit]       its length, 0..4096
 *   slot_unit  int64 [nslot + 1]   slot s owns the contiguous run of units [slot_unit[s], slot_unit[s + 1])
 *   Offsets are clamped into [0, n], lengths to 4096 and to n, unit indices into [0, nunit]: a malformed table gives wrong
 *   values, never an access outside [0, n) of g and p or outside the workspace.
 * Values: x = g * grad_scale in fp32; an element is NON-FINITE exactly as the guard defines it: x * x in fp32 is NaN or Inf.
 *   out_f  float [nslot][4]   [0] sum of x^2 over the slot's finite elements   [1] max |x| over them
 *                             [2] sum of p^2 over the slot                     [3] max |p| over the slot    (p NULL: both 0)
 *   out_i  int64 [nslot][2]   [0] number of non-finite elements (left out of out_f[.][0..1])   [1] number of elements with g == 0
 * Two passes, no float atomics; two launches on the same inputs give bitwise equal outputs, whatever the workspace held before:
 *   pass 1  one wave per unit (a fixed grid of waves striding over the units): a lane adds at most 64 terms in rising order, the
 *           unit's head and tail up to 16-byte alignment are scalar loads, the body 16-byte vector loads; the unit's partial result
 *           goes to the workspace (vacnic_param_stats_workspace_bytes(nunit, nslot) bytes, 16-byte aligned, owned by the caller)
 *   pass 2  one workgroup per slot folds the slot's run of partials in unit order (a thread takes every 256th) through a fixed tree
 * Gate, evaluated by both passes from the same device values:
 *   hyper  float[2] (may be NULL), hyper[1] = the step count after vacnic_lr_step: the 1-based number of this step
 *   every  >= 1;   skip  (may be NULL) the step word (vacnic_adamw_args.skip): the guard's state or vacnic_lr_step_accum's accum
 *   the call FIRES when hyper == NULL, or (int64)hyper[1] % every == 0, or skip != NULL && *skip == 1 — a dropped step always records
 *   its statistics (its hyper[1] is the count after the guard took the increment back).  *skip == 2 (a held micro-batch of an
 *   accumulation group) never fires, so `every` counts optimizer steps, as hyper[1] does.
 *   Not fired: nothing is written to out_f, out_i or stamp.
 *   Fired:     stamp int64[4] = {fires so far (incremented), (int64)hyper[1] as read (-1 if NULL), 1 if *skip != 0 else 0, 0};
 *              the caller zeroes stamp once.
 * Status 1..3 with a message, before any launch, for: a null g / table / workspace / output, n < 0, nslot < 1, nunit < 1,
 * every < 1, a workspace that is too small, misaligned operands.
 */
typedef struct {
  const float* g; const float* p; int64_t n; float grad_scale;
  const int64_t* unit_off; const int32_t* unit_len; int64_t nunit;
  const int64_t* slot_unit; int64_t nslot;
  const float* hyper; int32_t every; const int64_t* skip;
  void* workspace; int64_t workspace_bytes;
  float* out_f; int64_t* out_i; int64_t* stamp;
} vacnic_param_stats_args;
int vacnic_param_stats(const vacnic_param_stats_args* a, void* stream);
int64_t vacnic_param_stats_workspace_bytes(int64_t nunit, int64_t nslot);
/* get_linear_schedule_with_warmup on device (TRAIN:99-107): hyper[0] <- base_lr*lambda(k), hyper[1] <- k+1
 * where k = hyper[1] on entry = optimizer steps already taken.  Also increments *rng_counter (the device-side
 * dropout counter, may be NULL).  Call once before vacnic_adamw. */
int vacnic_lr_step(float* hyper, float base_lr, float warmup_steps, float total_steps, uint64_t* rng_counter, void* stream);
/* vacnic_lr_step for gradient accumulation: k micro-batches per optimizer step, counted on the device, so that every micro-batch
 * issues the same launches (backward accumulates into the fp32 gradient arena; the optimizer passes read the step word and act
 * on the group's last micro-batch only).
 *   accum  int64[4] = {step word, micro-batches pending, groups completed, 0}; the caller zeroes it once.
 * Every call increments *rng_counter (each micro-batch draws fresh dropout masks).  Then
 *   pending + 1 <  k:  pending += 1, step word = 2 (hold); hyper is untouched: neither the schedule position nor Adam's t moves
 *   otherwise:         pending = 0, groups += 1, step word = 0 (apply); hyper advances exactly as in vacnic_lr_step
 * Pass accum as `hold` to vacnic_grad_guard / vacnic_grad_clip_coef_groups, and as `skip` to vacnic_param_stats and vacnic_adamw*
 * (with a guard: its state, which carries the hold on).  Callers scale the gradient by 1 / k (grad_scale): the mean of the k
 * micro-batch gradients.  k == 1 is vacnic_lr_step bit for bit.  k < 1: status 1 before any launch. */
int vacnic_lr_step_accum(float* hyper, float base_lr, float warmup_steps, float total_steps, uint64_t* rng_counter, int64_t* accum,
                         int32_t k, void* stream);

/* ---- small data-movement helpers on the path ------------------------------------------------- */
/* f32 -> bf16 cast (weight shadow refresh, inputs). */
int vacnic_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream);
int vacnic_cast_bf16_f32(const void* src, float* dst, int64_t n, void* stream);
/* strided 2-D bf16 copy: dst[r*ldd + c] = src[r*lds + c], used for torch.cat along tokens
 * (MFULL:666,691) without materialising intermediates; accumulate=1 adds instead (cat backward). */
int vacnic_copy2d_bf16(const void* src, void* dst, int64_t rows, int64_t cols, int64_t lds, int64_t ldd,
                       int32_t accumulate, void* stream);
/* 3-D variant: [B][rows][cols] with batch strides. */
int vacnic_copy3d_bf16(const void* src, void* dst, int64_t B, int64_t rows, int64_t cols,
                       int64_t lds, int64_t ldd, int64_t bss, int64_t bsd, int32_t accumulate, void* stream);
/* dst[R][Cp] = src[R][C] zero-padded on the right (C not a multiple of 8: the 20-wide name-prefix FFN output,
 * MFULL:595) so the following GEMMs see 16-byte rows. */
int vacnic_pad_cols_bf16(const void* src, void* dst, int64_t R, int64_t C, int64_t Cp, int64_t lds, void* stream);
/* CLIP patch embedding im2col (conv1 with kernel = stride = patch, no bias; TRAIN:225-227):
 * img f32 [B][3][HW][HW] -> patches bf16 [B*g*g][Kp] (k = c*p*p + py*p + px, zero-padded to Kp). */
int vacnic_im2col_patches(const float* img, void* patches, int64_t B, int64_t HW, int64_t patch, int64_t Kp,
                          void* stream);
/* x[b][0] = cls + pos[0]; x[b][1+i] = patch_emb[b][i] + pos[1+i]  (TRAIN:228-229), bf16 out. */
int vacnic_vit_assemble(const void* patch_emb, const void* cls, const void* pos, void* out,
                        int64_t B, int64_t G2, int64_t W, void* stream);
/* int64 ids != pad -> uint8 mask, plus shift_tokens_right (TRAIN:196-217) in one launch. */
int vacnic_prep_ids(const int64_t* ids, uint8_t* mask, int64_t* shifted, int64_t B, int64_t T,
                    int64_t pad_id, int64_t start_id, void* stream);
/* face mask = (face_emb[:, :, -1] != 1) as uint8 (TRAIN:269; pad faces are all-ones rows, DSG:48,124). */
int vacnic_face_mask(const float* faces, uint8_t* mask, int64_t BF, int64_t D, void* stream);
/* out[B, na+nb] = cat(a[B,na], b[B,nb], dim 1) on bytes: fm = torch.cat((face_mask, name_mask), dim=1), MFULL:1262 */
int vacnic_cat2_u8(const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t B, int64_t na, int64_t nb, void* stream);
/* per-row argmax over V logits (greedy decode / eval_epoch TRAIN:424): lowest index wins ties. */
int vacnic_argmax_rows(const void* logits, int64_t* out, int64_t R, int64_t V, int64_t ldl,
                       int32_t logits_f32, void* stream);
/* sum of bias gradient: dbias[n] += sum_m dy[m][n]  (bf16 dy, f32 atomics). */
int vacnic_bias_grad(const void* dy, float* dbias, int64_t M, int64_t N, int64_t ldy, void* stream);
/* out = a + b (bf16) — gradient fan-in where a tensor feeds two consumers */
int vacnic_add_bf16(const void* a, const void* b, void* out, int64_t n, void* stream);

/* ---- decode (transformers 4.18 GenerationMixin.beam_search driven at TRAIN:513-520, DDPINF:758-842) ---- */
/*
 * Bad-word table (transformers 4.18 NoBadWordsLogitsProcessor), device memory, shared by vacnic_beam_init / vacnic_beam_step and
 * vacnic_sample_step: bad_words int32 [n_bad][VACNIC_BAD_WORD_LEN], word w in its row's first bad_len[w] entries (the rest -1),
 * bad_len int32 [n_bad], 1 <= bad_len[w] <= VACNIC_BAD_WORD_LEN.  n_bad = 0 (NULL tables) = off; n_bad > VACNIC_BAD_WORDS_MAX is
 * refused with VACNIC_UNSUPPORTED.  With a row's history h[0 .. cur_len - 1] (its decoder input so far, INCLUDING the start token), a
 * word of m tokens bans its last token w[m - 1] for the next position iff m - 1 <= cur_len and h[cur_len - (m - 1) + k] == w[k] for
 * every 0 <= k < m - 1 (4.18's _tokens_match): a one-token word is banned at every position, and a prefix as long as the WHOLE
 * history matches.  A banned token scores -inf; it joins the NoRepeatNGram bans and the MinLength suppression in one set, and a
 * forced position overrides all of them.  Ids outside [0, V) and lengths outside [1, VACNIC_BAD_WORD_LEN] in the table are skipped.
 */
#define VACNIC_BAD_WORDS_MAX 1024
#define VACNIC_BAD_WORD_LEN 16
/* Per beam row: log_softmax(logits[:V]) -> NoRepeatNGram bans (bans int32 [R][n_ban], -1 = none) -> MinLength
 * (suppress_eos) -> ForcedEOS (forced_token >= 0: that token scores 0, all others -inf) -> + beam_scores[r] ->
 * top-K (sorted, ties broken towards the lower token id).  top_val f32 [R][K], top_idx int32 [R][K]. */
int vacnic_beam_topk(const void* logits, const float* beam_scores, const int32_t* bans, int32_t n_ban, int32_t eos,
                     int32_t suppress_eos, int32_t forced_token, float* top_val, int32_t* top_idx, int64_t R, int64_t V,
                     int64_t ldl, int32_t K, int32_t logits_f32, void* stream);
/*
 * vacnic_beam_topk with the repetition penalty (transformers 4.18 RepetitionPenaltyLogitsProcessor).  The first fields are the
 * arguments of vacnic_beam_topk; with penalty_rule == 0 the call IS vacnic_beam_topk.  Otherwise history int32 [R][hist_stride]
 * holds row r's decoder input so far in its first cur_len entries, INCLUDING the start token (for BART the eos id: eos is penalised
 * from position 1, as in HF), 1 <= cur_len <= min(hist_stride, 1024), and P = penalty is a finite number > 0 (P < 1 rewards
 * repetition).  pen(x) = x < 0 ? x * P : x / P is ONE IEEE-754 fp32 operation, applied to every DISTINCT history token j in
 * [0, V) once, however often j occurs:
 *   penalty_rule 1, on the logits (HF greedy_search / sample run the processors on raw logits; generate() uses it for one beam):
 *     z'_j = pen(z_j) before anything else; the log-softmax, the bans, the beam score and the top-K all see z'.
 *   penalty_rule 2, on the scores (HF beam_search runs the processors on log_softmax(logits); generate() uses it for > 1 beam):
 *     s_j = z_j - lse(z) with the log-sum-exp of the UNPENALISED row (history tokens included), s'_j = pen(s_j); then the bans,
 *     then + beam_scores[r] (each of the three a separately rounded fp32 operation), then the top-K.
 * A banned or suppressed token scores -inf whatever its penalty; a forced position ignores the penalty.  Order of the result as in
 * vacnic_beam_topk (score desc, token asc) — under rule 2 over the final scores, and entries behind the last finite score read
 * (-inf, -1) there, whichever kernel serves the shape (a forced position reads as in vacnic_beam_topk).  -inf stays -inf.
 * VACNIC_BAD_SHAPE: as vacnic_beam_topk; penalty_rule outside 0 .. 2; with a rule: history NULL, P not a finite number > 0, cur_len
 * outside [1, hist_stride].  VACNIC_UNSUPPORTED: cur_len > 1024 with a rule.
 */
typedef struct {
  const void* logits; const float* beam_scores; const int32_t* bans; float* top_val; int32_t* top_idx; const int32_t* history;
  int64_t R, V, ldl, hist_stride;
  int32_t n_ban, eos, suppress_eos, forced_token, K, logits_f32, cur_len, penalty_rule;
  float penalty;
} vacnic_beam_topk_args;
int vacnic_beam_topk_ex(const vacnic_beam_topk_args* a, void* stream);
/*
 * LM head + vacnic_beam_topk of the single-token decoder fused (MFULL:1997 `lm_head(outputs[0]) + final_logits_bias`, then the
 * log_softmax -> processors -> + beam_scores -> topk of beam_search above): R <= 8 rows, d_model <= 1024.  The [R][V] logits never
 * reach HBM unless `logits` (fp32 [R][ldl], optional: diagnostics) is given (matrix-core product, fp32 accumulation).
 *   h bf16 [R][d] contiguous (final hidden rows); emb bf16 [V][ldw]; bias fp32 [V] or NULL; bans / beam_scores / eos / suppress_eos /
 *   forced_token / top_val / top_idx as in vacnic_beam_topk with K = K2 (n_ban = row length of bans).
 *   workspace: vacnic_lmhead_topk_workspace(R, V, K2) floats of caller-owned scratch (per-workgroup partial results).
 *   forced_token >= 0: no logits are computed (h / emb / workspace may be NULL): the forced token scores beam_scores[r], the rest -inf.
 *   vacnic_lmhead_topk_supported(R, V, d, K2): 1 if the call accepts this shape, else 0 (VACNIC_UNSUPPORTED): 1 <= R <= 8, d a multiple
 *   of 8 up to 1024, V <= 65536, K2 <= min(64, V), and the merge's G x K2 candidates (8 bytes each, G = workgroups of the part kernel,
 *   449 at V = 50265) fit the 160 KiB of LDS: K2 <= 45 at V = 50265.  Callers choose between this call and the GEMM -> vacnic_beam_topk
 *   chain with it.
 *   history / hist_stride / cur_len / penalty_rule / penalty: the repetition penalty exactly as in vacnic_beam_topk_ex (0 / NULL =
 *   off; the optional logits output stays unpenalised).  penalty_rule 2 needs R * hist_stride more floats of workspace behind the
 *   vacnic_lmhead_topk_workspace(R, V, K2) ones.  A penalty changes neither the shapes the call accepts nor
 *   vacnic_lmhead_topk_supported.
 */
typedef struct {
  const void* h; const void* emb; const float* bias; float* logits; float* workspace;
  const float* beam_scores; const int32_t* bans; float* top_val; int32_t* top_idx;
  int64_t R, V, d, ldw, ldl, workspace_floats;
  int32_t n_ban, eos, suppress_eos, forced_token, K2;
  int32_t cur_len, penalty_rule; float penalty;
  const int32_t* history; int64_t hist_stride;
} vacnic_lmhead_topk_args;
int64_t vacnic_lmhead_topk_workspace(int64_t R, int64_t V, int32_t K2);
int32_t vacnic_lmhead_topk_supported(int64_t R, int64_t V, int64_t d, int32_t K2);
int vacnic_lmhead_topk(const vacnic_lmhead_topk_args* a, void* stream);
/*
 * On-device beam-search bookkeeping: what transformers 4.18 BeamSearchScorer.process does on the host between
 * two decoder steps (TRAIN:513-520 -> GenerationMixin.beam_search), plus the NoRepeatNGram ban lists of the next position —
 * so the decode loop needs no device->host copy per token; the host reads this state once after the last position.
 * R = B * nb rows.  seq[k]: int32 [R][Lmax] token histories (position t reads seq[(t) & 1]... see beam_step), ping-pong.
 * Finished hypotheses are kept per batch item in list order: hyp_score f64 [B][nb] (= sum_logprobs / len^length_penalty),
 * hyp_len int32 [B][nb], hyp_seq int32 [B][nb][Lmax], hyp_cnt int32 [B], hyp_worst f64 [B]; done int32 [B].
 * vacnic_beam_init: histories = [start], beam scores = [0, -1e9, ...], empty lists.
 * vacnic_beam_step(cur_len): consumes beam_topk's [R][K2] candidates of the position whose histories hold cur_len tokens
 * (seq[(cur_len-1)&1]) and writes seq[cur_len&1], beam_scores (the next beam_topk's input), next_ids (last tokens, int64 [R]),
 * src_idx (int64 [R]: the row each new beam continues = KV-cache reorder index) and bans (int32 [R][Lmax + n_bad], -1 padded; NULL
 * if no_repeat_ngram_size == 0 and n_bad == 0).
 * bad_words / bad_len / n_bad (the table above; 0 / NULL = off): the bad-word bans of the NEXT position are appended to each row's
 * ban list behind the NoRepeatNGram bans (the same token may appear twice; the order inside a list is unspecified), one-token words
 * included, so the top-k kernels need nothing but `bans` with n_ban = Lmax + n_bad.  vacnic_beam_init writes the first position's
 * (history = [start]).  As with the n-gram bans, the rows of a finished batch item ban nothing.  n_bad > 0 with bans == NULL:
 * VACNIC_BAD_SHAPE.
 */
typedef struct {
  int32_t* seq[2]; float* beam_scores; int32_t* done; int32_t* hyp_cnt; double* hyp_worst; double* hyp_score; int32_t* hyp_len;
  int32_t* hyp_seq; int64_t* next_ids; int64_t* src_idx; int32_t* bans;
  int64_t B, nb, Lmax, V, eos, pad, no_repeat_ngram_size, early_stopping;
  float length_penalty;
  const int32_t* bad_words; const int32_t* bad_len; int64_t n_bad;
} vacnic_beam_state;
int vacnic_beam_init(const vacnic_beam_state* st, int32_t start_token, void* stream);
int vacnic_beam_step(const vacnic_beam_state* st, const float* top_val, const int32_t* top_idx, int32_t K2, int32_t cur_len,
                     void* stream);
/*
 * Group (diverse) beam search: transformers 4.18 GenerationMixin.group_beam_search with HammingDiversityLogitsProcessor
 * (generate(num_beam_groups=G, diversity_penalty=lambda)) on the state of vacnic_beam_init / vacnic_beam_step.  The nb beams of a batch
 * item are G groups of gs = nb / G: row r = b * nb + g * gs + i is slot i of group g.  The hypothesis list (capacity nb) and the done
 * flag stay ONE per batch item, shared by its groups, as 4.18's BeamSearchScorer keeps them (later transformers versions keep a list
 * per group; this is not that).  The top-k kernels run once per position over all R rows exactly as for ordinary beams; the groups
 * are handled inside ONE launch of vacnic_group_beam_step, one workgroup per batch item, group after group.
 *
 * vacnic_group_beam_init: vacnic_beam_init, but slot 0 of EVERY group starts live: beam_scores[r] = 0 for i == 0, else -1e9.
 * vacnic_group_beam_step(cur_len): per batch item b, for g = 0 .. G - 1 in order, with new_tok[] the tokens chosen so far in this
 * position:
 *   1. done[b] set (on entry, or by an earlier group of this position): the group's gs rows get score 0, token pad,
 *      src_idx = b * nb + g * gs, and ban nothing.  Next group.
 *   2. Hamming term, for every candidate (v, tok), tok >= 0, of the group's rows: f = #{rows r' of item b in groups < g with
 *      new_tok[r'] == tok} (a bincount: two earlier beams with the same token count twice).  If f > 0 and forced_token < 0:
 *      h = fp32(lambda * f); if penalty_rule == 2 and tok occurs in the row's history seq_in[r][0 .. cur_len): h = fp32(h * P);
 *      v' = fp32(v - h).  Otherwise v' = v.  A forced position (ForcedBOS / ForcedEOS, forced_token >= 0) skips the term: in HF the
 *      forced processors run after Hamming and overwrite its result.  The factor P is HF's processor order (Hamming, then
 *      RepetitionPenalty) on log-softmax scores s <= 0: pen(s - lambda f) = (s - lambda f) P = pen(s) - lambda f P.  Rounding: HF
 *      computes (s - lambda f) + beam_score, this computes (s + beam_score) - lambda f: they differ by at most the last bit.
 *   3. Merge: the group's candidates ordered (v' desc, i * V + tok asc), the best min(2 gs, K2) kept (G == 1: K2, as
 *      vacnic_beam_step keeps them).
 *   4. BeamSearchScorer.process with group_size = gs over those in rank order: EOS at rank >= gs is skipped; EOS at rank < gs adds
 *      (history of its row, v') to the item's shared list, scored (double)v' / cur_len^length_penalty (the host's pow); any other
 *      candidate continues, until gs continue.
 *   5. done[b] |= (list length >= nb) && (early_stopping || worst >= best_v' / cur_len^length_penalty), best_v' = rank 0 of THIS
 *      group's merged list.
 *   6. The group's rows: history (source row's + token), beam_scores, next_ids, src_idx (always a row of the same group), and the
 *      NoRepeatNGram / bad-word bans of the next position exactly as vacnic_beam_step writes them.
 * Why the per-row lists of K2 = min(2 nb, V) suffice (the top-k kernels need no change): the term only lowers scores, and lowers at
 * most nb - gs distinct tokens per row, so a row's list of 2 nb still holds at least nb + gs >= 2 gs unlowered entries; each of those
 * is at least as large as any unlisted token of the row, and on equal score the listed token has the lower id.  So the group's true
 * top 2 gs after the penalty lies inside the union of its rows' lists.
 * With num_beam_groups == 1 both calls leave the state bit for bit as vacnic_beam_init / vacnic_beam_step do (diversity_penalty,
 * repetition_penalty, penalty_rule and forced_token are then unused but still checked).
 * Shapes: those of vacnic_beam_step (nb <= 16, nb * K2 <= 128, Lmax <= 512; otherwise VACNIC_UNSUPPORTED).  VACNIC_BAD_SHAPE: as
 * vacnic_beam_init / vacnic_beam_step; num_beam_groups < 1 or not dividing nb; diversity_penalty negative or not finite;
 * repetition_penalty not a finite number > 0; penalty_rule outside {0, 2}.  All decided before any launch.
 */
typedef struct {
  int32_t num_beam_groups;      /* G */
  float diversity_penalty;      /* lambda >= 0; 0 = groups without the Hamming term */
  float repetition_penalty;     /* P of the top-k call of this position (read only under penalty_rule 2) */
  int32_t penalty_rule;         /* 0 = no repetition penalty, 2 = on the scores (vacnic_beam_topk_ex) */
  int32_t forced_token;         /* forced_token of the top-k call of this position (-1 = none) */
} vacnic_group_beam_args;
int vacnic_group_beam_init(const vacnic_beam_state* st, const vacnic_group_beam_args* ga, int32_t start_token, void* stream);
int vacnic_group_beam_step(const vacnic_beam_state* st, const vacnic_group_beam_args* ga, const float* top_val, const int32_t* top_idx,
                           int32_t K2, int32_t cur_len, void* stream);
/*
 * Sampling decode, one position (transformers 4.18 GenerationMixin.sample: processors on the raw logits, then the warpers
 * temperature -> top-k -> top-p, then softmax and one draw) with the bookkeeping of the position: one launch, one workgroup per
 * row, no host round trip.  Everything below is exact enough to be replayed on the host (tests/test_sample.py does).
 *
 * Inputs.  logits fp32 [R][ldl], the first V columns are real.  seq int32 [R][Lmax]: row r's history, cur_len tokens long
 * (1 <= cur_len < Lmax).  done int32 [R].  params: 8 32-bit words of DEVICE memory, read at run time so that a captured launch
 * serves every setting: [0] temperature T (f32)  [1] top_k (i32)  [2] top_p (f32)  [3] repetition penalty P (f32)  [4],[5] seed
 * (low, high word)  [6],[7] call counter (low, high word).  A T that is not > 0 is read as 1; a P that is not > 0 (the 0 of a
 * block written without one) is read as 1 = off.  bad_words / bad_len / n_bad: the bad-word table above (0 / NULL = off).
 *
 * Per row r, in this order:
 * 1. Processors.  done[r] != 0: the row writes `pad` (log-prob 0) and nothing else happens to it.  forced_token >= 0: that token is
 *    chosen with probability 1 (log-prob 0, kept = 1, thr = 0, mass = 1).  Otherwise token j becomes -inf if suppress_eos != 0 and
 *    j == eos (MinLength), or, with n = no_repeat_ngram_size > 0 and cur_len + 1 >= n, if j == seq[r][i + n - 1] for some
 *    0 <= i <= cur_len - n with seq[r][i .. i + n - 2] == seq[r][cur_len - n + 1 .. cur_len - 1] (NoRepeatNGram, computed from the
 *    history in place), or if the bad-word table bans it for this history (the rule above, also computed in place).  Before the
 *    bans, with P != 1 (RepetitionPenaltyLogitsProcessor on the raw logits, as HF's sample runs it): every DISTINCT token j of the
 *    history seq[r][0 .. cur_len - 1] (start token included, so BART's eos is penalised from position 1) has its logit replaced by
 *    z_j < 0 ? z_j * P : z_j / P — ONE IEEE-754 fp32 multiplication or division, applied once however often j occurs; for these
 *    tokens NaN is read as -inf and +inf as FLT_MAX first; -inf stays -inf.  P < 1 rewards repetition.  Everything below (steps 2-6,
 *    the reported log-prob included) sees the penalised logits.  A NaN logit counts as -inf, +inf as FLT_MAX.  A row without a
 *    finite logit left emits `eos` (log-prob 0, kept = 0) and finishes.
 * 2. Temperature.  z' = z / T: ONE IEEE-754 fp32 division, round to nearest even (not a multiplication by a reciprocal);
 *    -0 is read as +0.
 * 3. Top-k.  With 1 <= top_k < V: thr_k = the top_k-th largest z' counting duplicates and -inf entries; every z' >= thr_k stays,
 *    so ties at the k-th value are all kept (HF: `scores < topk[-1]` is removed).  top_k <= 0 or >= V: off.  Integer radix select
 *    over order-preserving keys: no floating-point arithmetic, the result is exact.
 * 4. Top-p.  With 0 < top_p < 1, over the tokens left by step 3: q_v = rint(exp(z'_v - max z') * 2^31) as an integer (expf in fp32,
 *    q = 0 for -inf), E_v = sum of q_w over the left tokens with z'_w > z'_v (STRICTLY larger), Zl = sum of all q_w.  Token v stays iff
 *    E_v <= floor((double)top_p * (double)Zl).  The top token always stays; tokens of equal z' stay or go together, so the kept set
 *    is {v : z'_v >= thr} for one threshold thr, found by a mass-weighted radix select over the whole row.  top_p >= 1 (or <= 0): off.
 *    Without ties this is HF's TopPLogitsWarper (sort descending, drop where the cumulative probability BEFORE the token exceeds top_p).
 * 5. Draw.  Philox4x32-10 with the 64-bit key K = seed + 0x9E3779B97F4A7C15 * call (mod 2^64; key word 0 = low half, word 1 = high
 *    half) and the counter words (r, cur_len, 0x53414D50, 0).  m = output word 0 >> 8, u = (m + 0.5) * 2^-24 = (2 m + 1) / 2^25.
 *    Over the kept FINITE tokens in ascending token id, with the integer masses q of step 4 (computed the same way when top-p is
 *    off) and Z their sum: the token is the first whose inclusive cumulative mass c satisfies c * 2^25 > (2 m + 1) * Z.
 *    All sums are integer sums, so they do not depend on the order they are formed in: two launches give the same bits, and there
 *    is no floating-point atomic.  (The masses differ from exact probabilities by < 2^-32 of the top token's each, plus expf's error.)
 * 6. Bookkeeping.  next_ids[r] (int64) = seq[r][cur_len] = token; done[r] = 1 if token == eos; logp[r][cur_len] (fp32 [R][Lmax],
 *    may be NULL) = (z'_token - max z') - log(Z / 2^31), the log-probability under the distribution the token was drawn from.
 *    Optional diagnostics (NULL = not written): kept[r] int32 = number of kept finite tokens; thr[r] = the threshold z' (-inf if
 *    nothing was cut); mass[r] = Z / Zl (1 when top-p is off); u[r] = fp32(u), round to nearest even (written for every row).
 *    u itself lies in (0, 1), but 2 m + 1 needs 25 bits once m >= 2^23 and fp32 holds 24: there the copy is rounded, and for
 *    m = 2^24 - 1 it reads exactly 1.0.  Only this diagnostic is rounded: the draw compares the integers above.
 * VACNIC_UNSUPPORTED: V outside [1, 65536], n_bad outside [0, VACNIC_BAD_WORDS_MAX].  VACNIC_BAD_SHAPE: a null operand (a table
 * pointer with n_bad > 0 included), R < 1, ldl < V, cur_len outside [1, Lmax), forced_token >= V, a negative n-gram size.
 */
typedef struct {
  const float* logits; const void* params; int32_t* seq; int32_t* done; int64_t* next_ids; float* logp;
  int32_t* kept; float* thr; float* mass; float* u;
  int64_t R, V, ldl, Lmax;
  int32_t cur_len, eos, pad, no_repeat_ngram_size, suppress_eos, forced_token;
  const int32_t* bad_words; const int32_t* bad_len; int32_t n_bad;
} vacnic_sample_step_args;
int vacnic_sample_step(const vacnic_sample_step_args* a, void* stream);
/*
 * Persistent single-token decoder step: every BartDecoderLayer of one position (MFULL:793-890 with
 * past_key_value, eval mode: self-attention over the KV cache, cross-attention over the encoder K/V projected once, FFN, the
 * three post-LayerNorms) in ONE launch of max(d / 4, ffn / 16) co-resident workgroups.  The 8 phases of a layer hand their
 * results over through tagged 16-byte units in the `slots` buffer (no grid barriers); the next projection's weights are
 * prefetched into LDS while a workgroup waits for its inputs.  R <= 8 rows (beams x batch), d_model <= 1024 with 64-wide heads,
 * ffn_dim <= 4096, d and ffn multiples of 16, L <= 120, max(d / 4, ffn / 16) <= min(256, CUs) and R x heads <= that count.
 * The projections run on the matrix cores: their fp32 sums associate differently from the kernel-per-op chain
 * vacnic_gemv_ln_bf16 / vacnic_gemm_bf16 (skinny) / vacnic_attn_fwd (Tq = 1), so results agree with it to bf16 tolerance, not
 * to the bit.
 *   layers   DEVICE array [L] of vacnic_decoder_layer: bf16 weights row-major [N][K] contiguous (w_kvq = k|v|q stacked, [3d][d]),
 *            fp32 biases and LayerNorm parameters; cross_kv bf16 [rows][S][2d] (k|v per source position) with cross_bs
 *            elements between rows (0: all rows share one source — the beams of one caption).
 *   cache    bf16 [L][R][Tmax + 1][2d]: k|v of position t are written at [l][r][t][0:2d] (the extra position is where the
 *            kernel-per-op chain parks q).
 *   h0       bf16 [R][d]: embedding LayerNorm output of the new token (vacnic_embed_ln_fwd).
 *   obuf     bf16 [R][d]: on return the decoder's final hidden rows (final_layer_norm of the last layer applied), ready for
 *            the LM-head GEMM.
 *   sync     vacnic_decoder_step_sync_bytes() bytes, zeroed ONCE by the caller; word [sync_bytes / 4 - 64] is an error flag the
 *            kernel raises (and leaves) if a wait times out — check it when the results are read back, and zero sync and slots
 *            again before the next launch if it is set.
 *   slots    vacnic_decoder_step_slots_bytes(L) bytes, zeroed ONCE by the caller: the phases' exchange buffer.
 */
typedef struct {
  const void *w_kvq, *w_so, *w_cq, *w_co, *w_fc1, *w_fc2;
  const float *b_kvq, *b_so, *b_cq, *b_co, *b_fc1, *b_fc2;
  const float *ln_self_g, *ln_self_b, *ln_cross_g, *ln_cross_b, *ln_final_g, *ln_final_b;
  const void* cross_kv;
  int64_t cross_bs;
} vacnic_decoder_layer;
typedef struct {
  const vacnic_decoder_layer* layers;
  void* cache; const void* h0;
  void* obuf;
  const uint8_t* enc_mask;        /* uint8 [R][S], 0 = masked source position; may be NULL */
  uint32_t* sync;
  void* slots;
  int64_t L, R, d, H, F, S, t, Tmax;
  float eps, scale;
  uint64_t* trace; int64_t trace_wg;   /* profiling aid, normally NULL: 100 MHz time stamps of workgroup trace_wg, uint64 [8 L + 1][8]
                                          ([phase][1] inputs gathered, [2] LayerNorm applied, [3] results packed; [8 L][4] / [6]
                                          wall clock and [5] / [7] shader clock at the start / end of the launch) */
} vacnic_decoder_step_args;
int64_t vacnic_decoder_step_sync_bytes(void);
int64_t vacnic_decoder_step_slots_bytes(int64_t L);
int vacnic_decoder_step(const vacnic_decoder_step_args* a, void* stream);
/* dst[r][:row_bytes] = src[g][:row_bytes] for rows row_stride_bytes apart (0 = row_bytes; both multiples of 16): KV-cache beam
 * reorder (_reorder_cache, MFULL:2066-2074).  period == 0: g = idx[r]; period > 0: g = (r / period) * period + idx[r % period] —
 * one beam permutation idx[period] applied to every layer's block of rows.  Copying only the filled prefix of a cache row
 * (row_bytes < row_stride_bytes) halves the traffic of the reorder on average. */
int vacnic_gather_rows(const void* src, void* dst, const int64_t* idx, int64_t rows, int64_t row_bytes, int64_t row_stride_bytes,
                       int64_t period, void* stream);

/* ---- input pipeline ---- */
/* uint8 image [B][3][H][W] -> fp32 [B][3][H][W]: torchvision ToTensor (x / 255) then Normalize ((t - mean[c]) / std[c]) of
 * TRAIN:741-764, with an optional per-image horizontal flip (flip[b] != 0; RandomHorizontalFlip, TRAIN:762 — the caller draws
 * the coin).  IEEE divisions, so the result is bit-identical to the torch formula. */
int vacnic_image_u8_normalize(const uint8_t* src, const uint8_t* flip, float* dst, int64_t B, int64_t H, int64_t W,
                              float mean0, float mean1, float mean2, float std0, float std1, float std2, void* stream);

/*
 * Fused LM head + cross entropy: logits = h . E^T (+ final_logits_bias) (MFULL:1885,1997) into
 * CrossEntropyLoss(ignore_index) (TRAIN:287,816) WITHOUT materialising the [R, V] logits.
 *   vacnic_lmhead_ce_fwd      one GEMM whose epilogue reduces each 256-column tile of a row to an online-softmax pair
 *                             {max, sum exp} (part[R][part_tiles][2], part_tiles = ceil(V/256)) and picks the target logit
 *                             (tl[R]); a combine kernel writes row_lse[R] and ACCUMULATES loss_sum / count (both zeroed by
 *                             the call) over rows whose target != ignore_index.  loss = loss_sum / count.
 *   vacnic_lmhead_ce_rowp     rowp[R][2] = {row_lse, (target != ignore) * grad_out * grad_scale / count} for the backward.
 *   vacnic_lmhead_ce_dlogits  recomputes the logits of vocabulary columns [col0, col0 + ncols) and writes
 *                             dlogits = (softmax - onehot(target)) * rowp[.][1] as bf16 [R][lddl] (columns ncols..round_up(ncols,8)
 *                             are written as zeros); the caller runs the dh / dE GEMMs on the chunk and re-uses the buffer.
 * Domain of the targets: every target lies in [0, V) or equals ignore_index; anything else is undefined on the fused path (the
 * combine kernel only tests target != ignore_index, so an out-of-range target would read a tl[r] that no tile wrote).  The
 * materialised pair vacnic_ce_fwd / vacnic_ce_bwd treats every target outside [0, V) as ignored.
 * Label smoothing (label_smoothing = eps in [0, 1); anything else: VACNIC_BAD_SHAPE), torch's CrossEntropyLoss(label_smoothing=eps)
 * over the V real columns:  row_loss = (1 - eps) (lse - z_t) + eps (lse - mean_j z_j),
 *                           dlogits  = (softmax - (1 - eps) onehot(target) - eps / V) * coef.
 *   eps > 0: vacnic_lmhead_ce_fwd also needs part_sum[R][part_tiles] (the epilogue's per-tile sums of the valid logits), and
 *            vacnic_lmhead_ce_dlogits reads rowp as FOUR floats per row, 16-byte aligned, written by vacnic_lmhead_ce_rowp_smooth:
 *            rowp[R][4] = {row_lse, coef, coef * (1 - eps), coef * eps / V}.  row_lse does not depend on eps.
 *   eps == 0 (a zero-initialised tail of the struct): part_sum is not touched, rowp is the [R][2] array of vacnic_lmhead_ce_rowp, the
 *            kernels launched are the ones without the option: row_lse, count and dlogits are bit-identical to theirs; loss_sum is,
 *            as always, an fp32 atomic sum over the rows, equal up to the order of its additions.
 */
typedef struct {
  const void* h; const void* emb; const float* bias;      /* bf16 [R][ldh], bf16 [>=V][lde] (tied embedding), f32 [V] or NULL */
  const int64_t* targets;                                 /* [R] */
  float* part; float* tl; float* row_lse; float* loss_sum; float* count;
  int64_t R, V, D, ldh, lde, part_tiles, ignore_index;
  float* part_sum;                                        /* f32 [R][part_tiles] contiguous scratch (R * part_tiles floats, written with
                                                             4-byte stores: no alignment beyond a float's), label_smoothing > 0 only
                                                             (else may be NULL and is never read or written) */
  float label_smoothing;
} vacnic_lmhead_ce_args;
int vacnic_lmhead_ce_fwd(const vacnic_lmhead_ce_args* a, void* stream);
int vacnic_lmhead_ce_rowp(const float* row_lse, const int64_t* targets, const float* count, const float* grad_out,
                          float grad_scale, float* rowp, int64_t R, int64_t ignore_index, void* stream);
int vacnic_lmhead_ce_rowp_smooth(const float* row_lse, const int64_t* targets, const float* count, const float* grad_out,
                                 float grad_scale, float label_smoothing, int64_t V, float* rowp, int64_t R, int64_t ignore_index,
                                 void* stream);
int vacnic_lmhead_ce_dlogits(const vacnic_lmhead_ce_args* a, int64_t col0, int64_t ncols, void* dl, int64_t lddl,
                             const float* rowp, void* stream);

/*
 * Per-row weights on the fused LM head: loss = sum_r w_r l_r / N with w_r = weights[r / rows_per_weight] (rows_per_weight = 1: one
 * weight per token; = T: one per caption of T consecutive rows) and l_r the row's loss term of the unweighted path.  The GEMMs are
 * the unweighted ones: run vacnic_lmhead_ce_fwd as it is (its atomic loss_sum pointed at a word nobody reads), then
 *   vacnic_lmhead_ce_wloss   from row_lse, tl and (label_smoothing > 0) part_sum [R][part_tiles] of that call:
 *                            row_nll[r]   = l_r, the expression and tile-sum order of vacnic_lmhead_row_loss (bit-identical to its
 *                                           row_loss; an exact 0 where targets[r] == ignore_index),
 *                            row_wloss[r] = w_r * l_r, row_wnorm[r] = 1 (norm_mode 0, "tokens") or w_r (norm_mode 1, "weights"); both
 *                                           0 on ignored rows,
 *                            acc[0] = sum_r row_wloss[r], acc[1] = N = sum_r row_wnorm[r], each in the order of vacnic_sum_ordered
 *                            (256 strands, then ascending).  N is the number of non-ignored rows (norm_mode 0) or the sum of their
 *                            weights (norm_mode 1).
 *   vacnic_lmhead_ce_rowp_w  the rowp of vacnic_lmhead_ce_dlogits, [R][2] for label_smoothing == 0, else [R][4] (16-byte aligned), with
 *                            c = *norm, g = (grad_out ? *grad_out : 1) * grad_scale / c, coef = g * w_r in this order: w_r == 1.0f
 *                            gives the bits of vacnic_lmhead_ce_rowp / _rowp_smooth.  coef (1 - eps) and coef eps / V are formed from
 *                            that coef.  coef = 0 on ignored rows.  c is used as it is (no clamp to 1); c <= 0, NaN or inf makes every
 *                            coefficient 0: no gradient, and no NaN in the gradient arena.
 * loss = acc[0] / acc[1] (vacnic_combine_losses); 0 / 0 is NaN, like torch's mean over nothing.  Weights are any finite fp32 value,
 * negative ones included (advantages are signed).  A row with w_r == 0 contributes exactly what an ignored row contributes under
 * norm_mode 1; under norm_mode 0 it still counts as a token.  norm_mode 1 is meant for w >= 0.
 * No floating-point atomics and no memset: both calls are bit-reproducible, in the default and in the deterministic mode alike, and
 * record into launch plans and hipGraph captures.
 * VACNIC_BAD_SHAPE before any launch: a null operand (part_sum may be NULL without smoothing, grad_out always), rows_per_weight < 1 or
 * R % rows_per_weight != 0, norm_mode outside {0, 1}, label_smoothing outside [0, 1), smoothing without part_sum,
 * part_tiles != ceil(V / 256).
 */
int vacnic_lmhead_ce_wloss(const float* row_lse, const float* tl, const int64_t* targets, const float* part_sum, const float* weights,
                           int64_t rows_per_weight, int64_t R, int64_t V, int64_t part_tiles, int64_t ignore_index,
                           float label_smoothing, int32_t norm_mode, float* row_nll, float* row_wloss, float* row_wnorm, float* acc,
                           void* stream);
int vacnic_lmhead_ce_rowp_w(const float* row_lse, const int64_t* targets, const float* weights, int64_t rows_per_weight,
                            const float* norm, const float* grad_out, float grad_scale, float label_smoothing, int64_t V, float* rowp,
                            int64_t R, int64_t ignore_index, void* stream);

/*
 * Fused validation head: teacher-forced token log-probabilities, greedy predictions and per-caption sums from ONE LM-head pass,
 * again WITHOUT the [R, V] logits.  The forward GEMM of vacnic_lmhead_ce_fwd runs with a third epilogue (a kernel of its own; the
 * kernels vacnic_lmhead_ce_fwd launches are untouched): besides part[R][part_tiles][2] = {max, sum exp} and tl[R] it writes
 * part_arg[R][part_tiles], the GLOBAL column of each tile's largest logit among the valid columns n < V (after the bias; ties go
 * to the lowest column; the zero rows that pad the embedding beyond V never take part).  A combine kernel (one wave per row) writes
 *   row_lse[r]   bit-identical to vacnic_lmhead_ce_fwd's on the same operands,
 *   row_nll[r] = row_lse[r] - logit[r][target[r]], an exact 0 where target[r] == ignore_index,
 *   pred[r]      argmax_j logit[r][j] over j < V (larger value, then lower index), for ignored rows too;
 * a per-caption kernel sums each run of rows_per_seq consecutive rows in a fixed order:
 *   seq_nll[s] (f32), seq_tokens[s] = rows with target != ignore_index, seq_correct[s] = those of them with pred == target;
 * and, when totals != NULL, one workgroup adds this call's sums in index order onto the running record
 *   totals[4] (f64) += {sum seq_nll, sum seq_tokens, sum seq_correct, R / rows_per_seq}.
 * The caller zeroes totals once per validation pass with vacnic_zero_bytes; the call itself issues no memset (see
 * vacnic_zero_bytes: a memset node is unsafe under capture) and no floating-point atomic, so every output is bit-reproducible.
 * Scratch: part R * part_tiles * 2 floats, part_arg R * part_tiles int32, tl R floats; all contiguous, 4-byte stores.
 * Domain of the targets: as for vacnic_lmhead_ce_fwd, in [0, V) or equal to ignore_index.
 * VACNIC_BAD_SHAPE before any launch: a null operand (bias and totals may be NULL), R % rows_per_seq != 0,
 * part_tiles != ceil(V / 256).
 */
typedef struct {
  const void* h; const void* emb; const float* bias; const int64_t* targets;
  float* part; int32_t* part_arg; float* tl;                 /* scratch: [R][part_tiles][2], [R][part_tiles], [R] */
  float* row_lse; float* row_nll; int64_t* pred;             /* [R] */
  float* seq_nll; int32_t* seq_tokens; int32_t* seq_correct; /* [R / rows_per_seq] */
  double* totals;                                            /* [4], accumulated; may be NULL */
  int64_t R, V, D, ldh, lde, part_tiles, ignore_index, rows_per_seq;
} vacnic_lmhead_eval_args;
int vacnic_lmhead_eval(const vacnic_lmhead_eval_args* a, void* stream);

/* zero `bytes` bytes at `ptr` on `stream`: the fp32 accumulators of split-K GEMMs, the arrival counters of the split-K fix-up.
 * hipMemsetAsync on an ordinary stream; a fill kernel while `stream` is being captured into a hipGraph (a memset NODE is not
 * reliably ordered before the kernel node that follows it when the graph replays). */
int vacnic_zero_bytes(void* ptr, int64_t bytes, void* stream);

/* ---- launch plans: a step's C-ABI call sequence recorded once and replayed from C++ -----------------------------------------
 * The reference issues every kernel of a training step from Python (TRAIN:253-383); the eager path here does too (~1400 calls).
 * Between vacnic_plan_begin() and vacnic_plan_end(h) every entry point of this library also freezes its arguments into plan h
 * while it runs; vacnic_plan_replay(h, first, last) re-issues commands [first, last) — same kernels, same streams, same order.
 * The caller keeps all buffers at their recorded addresses and refreshes inputs in place.  vacnic_plan_mark() (while recording)
 * = index of the next command, for replays split around host-side work.  vacnic_stream_fence(src, dst): dst waits for all work
 * enqueued on src so far — the recordable form of an event record + stream wait.  vacnic_plan_pause(1) .. vacnic_plan_pause(0)
 * (recording thread only; nests): calls in between run but are NOT recorded — the work the host repeats itself at a mark of
 * every replay (the DDP reducer's bucket casts and RCCL launches, reference role TRAIN:87).  Recording is bound to the thread
 * that called vacnic_plan_begin, and an entry point that returns an error while recording leaves no command behind.
 * Handles are small integers; -1 = error. */
int64_t vacnic_plan_begin(void);
int vacnic_plan_end(int64_t plan);
int64_t vacnic_plan_size(int64_t plan);
int64_t vacnic_plan_mark(void);
int vacnic_plan_pause(int on);
int vacnic_plan_replay(int64_t plan, int64_t first, int64_t last);
int vacnic_plan_destroy(int64_t plan);
int vacnic_stream_fence(void* src_stream, void* dst_stream);

/* ---- data-parallel communication: RCCL behind the C-ABI ------------------------------------------------------------------------
 * The reference's DDP wrapper (torch.nn.parallel.DistributedDataParallel over NCCL, TRAIN:87) all-reduces gradient buckets from
 * C++ hooks; here a bucket's SUM all-reduce is a stream-ordered launch on a stream the caller names, recordable into a launch
 * plan like any kernel.  librccl is resolved with dlopen (vacnic_comm_load; path = NULL searches the usual names), so the
 * library loads on a box without RCCL and these entry points then return VACNIC_UNSUPPORTED.
 *   vacnic_comm_unique_id   rank 0: 128 opaque bytes to hand to every rank out of band (ncclGetUniqueId)
 *   vacnic_comm_init        every rank, with its GPU current: communicator handle >= 0, or -1 (ncclCommInitRank)
 *   vacnic_allreduce_bucket in-place SUM over the communicator, dtype 0 = f32, 1 = bf16 (ncclAllReduce)
 *   vacnic_comm_broadcast   in-place broadcast from `root` (the parameter broadcast at construction, TRAIN:87)
 *   vacnic_event_record / vacnic_event_wait   named events (slots 0 .. 511): the consumer stream waits for ONE point of the
 *                           producer stream (a bucket's all-reduce), whatever that stream is given afterwards */
int vacnic_comm_load(const char* librccl_path);
int vacnic_comm_unique_id(void* out128);
int64_t vacnic_comm_init(const void* id128, int rank, int world);
int vacnic_allreduce_bucket(int64_t comm, void* buf, int64_t count, int dtype, void* stream);
int vacnic_comm_broadcast(int64_t comm, void* buf, int64_t count, int dtype, int root, void* stream);
int vacnic_comm_destroy(int64_t comm);
int vacnic_event_record(int slot, void* stream);
int vacnic_event_wait(int slot, void* stream);

/* ---- hardware probes (tests only): verify MFMA / ds_read_tr lane maps assumed by the kernels -- */
int vacnic_probe_layouts(float* out, const float* src128, int64_t n_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
