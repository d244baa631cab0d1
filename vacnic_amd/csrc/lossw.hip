// Per-row weights on the fused LM-head cross entropy: loss = sum_r w_r l_r / N.  The GEMMs and their epilogues are untouched — the
// forward (vacnic_lmhead_ce_fwd) leaves row_lse, tl and (label smoothing) part_sum behind, the backward (vacnic_lmhead_ce_dlogits)
// multiplies every row by one coefficient of rowp.  The two calls here stand between them:
//   lmhead_ce_wloss  : l_r as vacnic_lmhead_row_loss forms it, w_r l_r and the row's share of N, then both sums in the fixed order of
//                      vacnic_sum_ordered (256 strands, then ascending) -> acc = {sum w l, N}
//   lmhead_ce_rowp_w : rowp[R][2] / [R][4] with coef = (grad_out * grad_scale / N) * w_r
// Plain grids, one writer per element, no atomics: the same bits in every run, whatever the mode.
#include "common.h"

// a * b + c stays a rounded product and a rounded sum (ordered.hip: l_r must have lmhead_row_loss_kernel's bits)
#pragma clang fp contract(off)

namespace {

constexpr int SUM_STRANDS = 256;       // the strand count of vacnic_sum_ordered

// one wave per row; the loss term is lmhead_row_loss_kernel's expression, tile sums in its order
__global__ __launch_bounds__(256) void lmhead_wloss_rows_kernel(const float* __restrict__ row_lse, const float* __restrict__ tl,
                                                                const int64_t* __restrict__ targets, const float* __restrict__ part_sum,
                                                                const float* __restrict__ weights, int64_t rows_per_weight,
                                                                float* __restrict__ row_nll, float* __restrict__ row_wloss,
                                                                float* __restrict__ row_wnorm, int R, int tiles, int64_t ignore, float eps,
                                                                float inv_v, int norm_mode) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  if (r >= R) return;
  float l = 0.f, wl = 0.f, wn = 0.f;
  if (targets[r] != ignore) {                      // (wave-uniform)
    l = row_lse[r] - tl[r];
    if (part_sum) {
      float zs = 0.f;
      for (int t = lane; t < tiles; t += 64) zs += part_sum[(size_t)r * tiles + t];
      const float mean = wave_sum(zs) * inv_v;
      const float term = eps * (tl[r] - mean);
      l = l + term;
    }
    const float w = weights[(int64_t)r / rows_per_weight];
    wl = w * l;
    wn = norm_mode ? w : 1.f;
  }
  if (lane == 0) { row_nll[r] = l; row_wloss[r] = wl; row_wnorm[r] = wn; }
}

// sum_ordered_kernel with two accumulators: strand t adds a[t], a[t + 256], ... ; thread 0 adds the strand sums in ascending order
__global__ __launch_bounds__(256) void sum2_ordered_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                           float* __restrict__ dst) {
  __shared__ float red[2][SUM_STRANDS];
  float sa = 0.f, sb = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += SUM_STRANDS) { sa += a[i]; sb += b[i]; }
  red[0][threadIdx.x] = sa;
  red[1][threadIdx.x] = sb;
  __syncthreads();
  if (threadIdx.x == 0) {
    float ta = 0.f, tb = 0.f;
    for (int i = 0; i < SUM_STRANDS; ++i) { ta += red[0][i]; tb += red[1][i]; }
    dst[0] = ta;
    dst[1] = tb;
  }
}

// g = grad_out * grad_scale / N as ce_rowp_kernel forms it (N used as it is, no clamp), then coef = g * w_r: w_r == 1 leaves g's bits.
// N <= 0, NaN or inf: every coefficient is 0.
__device__ __forceinline__ float rowp_w_coef(const float* norm, const float* grad_out, float grad_scale, const float* weights,
                                             int64_t rows_per_weight, const int64_t* targets, int r, int64_t ignore) {
  const float c = *norm;
  if (!(c > 0.f) || c == INFINITY || targets[r] == ignore) return 0.f;
  const float g = (grad_out ? *grad_out : 1.f) * grad_scale / c;
  return g * weights[(int64_t)r / rows_per_weight];
}

__global__ void ce_rowp_w_kernel(const float* __restrict__ row_lse, const int64_t* __restrict__ targets, const float* __restrict__ weights,
                                 int64_t rows_per_weight, const float* __restrict__ norm, const float* __restrict__ grad_out,
                                 float grad_scale, float* __restrict__ rowp, int R, int64_t ignore) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  rowp[2 * (size_t)r] = row_lse[r];
  rowp[2 * (size_t)r + 1] = rowp_w_coef(norm, grad_out, grad_scale, weights, rows_per_weight, targets, r, ignore);
}

__global__ void ce_rowp_w_smooth_kernel(const float* __restrict__ row_lse, const int64_t* __restrict__ targets,
                                        const float* __restrict__ weights, int64_t rows_per_weight, const float* __restrict__ norm,
                                        const float* __restrict__ grad_out, float grad_scale, float eps, float inv_v,
                                        float* __restrict__ rowp, int R, int64_t ignore) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float g = rowp_w_coef(norm, grad_out, grad_scale, weights, rows_per_weight, targets, r, ignore);
  *(f32x4*)(rowp + 4 * (size_t)r) = (f32x4){row_lse[r], g, g * (1.f - eps), g * eps * inv_v};
}

}  // namespace

extern "C" int vacnic_lmhead_ce_wloss(const float* row_lse, const float* tl, const int64_t* targets, const float* part_sum,
                                      const float* weights, int64_t rows_per_weight, int64_t R, int64_t V, int64_t part_tiles,
                                      int64_t ignore_index, float label_smoothing, int32_t norm_mode, float* row_nll, float* row_wloss,
                                      float* row_wnorm, float* acc, void* stream) {
  VPLAN_REC(vacnic_lmhead_ce_wloss, row_lse, tl, targets, part_sum, weights, rows_per_weight, R, V, part_tiles, ignore_index,
            label_smoothing, norm_mode, row_nll, row_wloss, row_wnorm, acc, stream);
  VCHECK(row_lse && tl && targets && weights && row_nll && row_wloss && row_wnorm && acc, VACNIC_BAD_SHAPE, "lmhead_ce_wloss: null operand");
  VCHECK(R > 0 && R < (1ll << 31) && V > 0, VACNIC_BAD_SHAPE, "lmhead_ce_wloss: empty problem");
  VCHECK(rows_per_weight >= 1 && R % rows_per_weight == 0, VACNIC_BAD_SHAPE, "lmhead_ce_wloss: R=%ld rows do not split into weights of %ld rows",
         (long)R, (long)rows_per_weight);
  VCHECK(norm_mode == 0 || norm_mode == 1, VACNIC_BAD_SHAPE, "lmhead_ce_wloss: norm_mode %d is neither 0 (tokens) nor 1 (weights)", (int)norm_mode);
  VCHECK(label_smoothing >= 0.f && label_smoothing < 1.f, VACNIC_BAD_SHAPE, "lmhead_ce_wloss: label_smoothing %g outside [0, 1)", (double)label_smoothing);
  const bool smooth = label_smoothing > 0.f;
  VCHECK(!smooth || part_sum, VACNIC_BAD_SHAPE, "lmhead_ce_wloss: label_smoothing > 0 needs part_sum [R][ceil(V / 256)] of vacnic_lmhead_ce_fwd");
  VCHECK(part_tiles == (V + 255) / 256, VACNIC_BAD_SHAPE, "lmhead_ce_wloss: part_tiles must equal ceil(V / 256) = %ld", (long)((V + 255) / 256));
  hipLaunchKernelGGL(lmhead_wloss_rows_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, row_lse, tl, targets,
                     smooth ? part_sum : nullptr, weights, rows_per_weight, row_nll, row_wloss, row_wnorm, (int)R, (int)part_tiles,
                     ignore_index, label_smoothing, 1.f / (float)V, (int)norm_mode);
  VLAUNCH_CHECK();
  hipLaunchKernelGGL(sum2_ordered_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_wloss, row_wnorm, R, acc);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int vacnic_lmhead_ce_rowp_w(const float* row_lse, const int64_t* targets, const float* weights, int64_t rows_per_weight,
                                       const float* norm, const float* grad_out, float grad_scale, float label_smoothing, int64_t V,
                                       float* rowp, int64_t R, int64_t ignore_index, void* stream) {
  VPLAN_REC(vacnic_lmhead_ce_rowp_w, row_lse, targets, weights, rows_per_weight, norm, grad_out, grad_scale, label_smoothing, V, rowp, R,
            ignore_index, stream);
  VCHECK(row_lse && targets && weights && norm && rowp, VACNIC_BAD_SHAPE, "lmhead_ce_rowp_w: null operand");
  VCHECK(R > 0 && R < (1ll << 31) && V > 0, VACNIC_BAD_SHAPE, "lmhead_ce_rowp_w: empty problem");
  VCHECK(rows_per_weight >= 1 && R % rows_per_weight == 0, VACNIC_BAD_SHAPE, "lmhead_ce_rowp_w: R=%ld rows do not split into weights of %ld rows",
         (long)R, (long)rows_per_weight);
  VCHECK(label_smoothing >= 0.f && label_smoothing < 1.f, VACNIC_BAD_SHAPE, "lmhead_ce_rowp_w: label_smoothing %g outside [0, 1)", (double)label_smoothing);
  const dim3 grid((unsigned)((R + 255) / 256));
  if (label_smoothing > 0.f) {
    VCHECK(aligned16(rowp), VACNIC_MISALIGNED, "lmhead_ce_rowp_w: the 4-float rowp of label smoothing must be 16-byte aligned");
    hipLaunchKernelGGL(ce_rowp_w_smooth_kernel, grid, dim3(256), 0, (hipStream_t)stream, row_lse, targets, weights, rows_per_weight, norm,
                       grad_out, grad_scale, label_smoothing, 1.f / (float)V, rowp, (int)R, ignore_index);
  } else {
    hipLaunchKernelGGL(ce_rowp_w_kernel, grid, dim3(256), 0, (hipStream_t)stream, row_lse, targets, weights, rows_per_weight, norm, grad_out,
                       grad_scale, rowp, (int)R, ignore_index);
  }
  VLAUNCH_CHECK();
  return VACNIC_OK;
}
