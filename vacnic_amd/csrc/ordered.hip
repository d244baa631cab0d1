// Fixed-order fp32 sums for the deterministic mode (ops.set_deterministic): every kernel here is a plain grid, every output
// element has exactly ONE writer (a plain read-modify-write, no atomics), and the order of every addition is a function of the
// shapes alone — documented in include/vacnic_hip.h, emulated add for add by tests/test_deterministic_gpu.py.  Nothing waits for
// another workgroup.
//
//   fold_ordered        : dst[c] += sum_b partials[b][c]                 (LayerNorm dgamma / dbeta, stage 2 of the bias gradient)
//   bias_grad_ordered   : dbias[n] += sum_m dy[m][n] in two stages       (replaces the xsum atomics / vacnic_bias_grad)
//   scatter_ordered     : demb[id] += scale * sum_{r: ids[r] == id} src[r], dpos[t] += sum_{r: r % T + off == t} src[r]
//   sum_ordered         : dst[0] = sum_i src[i]                          (loss_sum from the per-row loss terms)
//   lmhead_row_loss     : per-row loss terms of the fused LM head from what its forward left behind
#include "common.h"

// a * b + c must stay a rounded product and a rounded sum in every kernel of this file (one kernel contracting where another does
// not would be a one-ulp difference between two "identical" results)
#pragma clang fp contract(off)

namespace {

constexpr int FOLD_STRANDS = 4;        // include/vacnic_hip.h documents the orders below with these numbers
constexpr int SUM_STRANDS = 256;
constexpr int BIAS_MAX_ROW_BLOCKS = 256;

// grid (ceil(cols / 64), ndst): wave w of a block is strand w of 64 columns
__global__ __launch_bounds__(256) void fold_ordered_kernel(const float* __restrict__ partials, int64_t ld, float* __restrict__ dst,
                                                           float* __restrict__ dst2, int NB, int cols) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int k = blockIdx.y;
  float s = 0.f;
  if (c < cols) {
    const float* p = partials + (size_t)k * cols + c;
    int b = wave;
    for (; b + 7 * FOLD_STRANDS < NB; b += 8 * FOLD_STRANDS) {      // 8 loads in flight, added in ascending row order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(b + u * FOLD_STRANDS) * ld];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; b < NB; b += FOLD_STRANDS) s += p[(size_t)b * ld];
  }
  __shared__ float red[FOLD_STRANDS][64];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < cols) {
    float t = red[0][lane] + red[1][lane];
    t += red[2][lane];
    t += red[3][lane];
    float* d = k ? dst2 : dst;
    d[c] = d[c] + t;
  }
}

// stage 1 of the bias gradient: block (cb, rb) = 512 columns x rows [rb * rows_per_block, +rows_per_block); wave g adds rows
// r0 + g, r0 + g + 4, ... in ascending order, the four wave sums meet as ((g0 + g1) + g2) + g3 -> partials[rb][col]
__global__ __launch_bounds__(256) void bias_partial_kernel(const bf16_t* __restrict__ dy, float* __restrict__ partials, long M, int N,
                                                           long ldy, int rows_per_block) {
  __shared__ float red[4][64 * 8 + 1];
  const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;           // 8-col chunk
  const long r0 = (long)blockIdx.y * rows_per_block;
  const long r1 = min(M, r0 + rows_per_block);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (c * 8 + 8 <= N) {
    long r = r0 + rg;
    for (; r + 28 < r1; r += 32) {                // 8 rows per trip, all loads issued before the adds
      u32x4 d[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) d[u] = *(const u32x4*)(dy + (r + 4 * u) * ldy + c * 8);
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) { acc[2 * k] += __uint_as_float(d[u][k] << 16); acc[2 * k + 1] += __uint_as_float(d[u][k] & 0xffff0000u); }
    }
    for (; r < r1; r += 4) {
      const u32x4 d = *(const u32x4*)(dy + r * ldy + c * 8);
#pragma unroll
      for (int k = 0; k < 4; ++k) { acc[2 * k] += __uint_as_float(d[k] << 16); acc[2 * k + 1] += __uint_as_float(d[k] & 0xffff0000u); }
    }
  } else if (c * 8 < N) {
    for (long r = r0 + rg; r < r1; r += 4)
      for (int j = 0; j < 8; ++j) if (c * 8 + j < N) acc[j] += bf2f(dy[r * ldy + c * 8 + j]);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[rg][lane * 8 + j] = acc[j];
  __syncthreads();
  for (int e = threadIdx.x; e < 512; e += 256) {
    const int col = blockIdx.x * 512 + e;
    if (col < N) {
      float t = red[0][e] + red[1][e];
      t += red[2][e];
      t += red[3][e];
      partials[(size_t)blockIdx.y * N + col] = t;
    }
  }
}

__device__ __forceinline__ int64_t clamp_id(int64_t id, int64_t V) { return id < 0 ? 0 : (id >= V ? V - 1 : id); }

// One block per source row r.  A pad row leaves at once; so does a row whose (clamped) id occurs in an earlier non-pad row.  The
// first row of an id walks the ids behind it, 256 at a time, and adds the rows of the same id in ascending order — the matches of a
// chunk are known from a ballot before the first of them is loaded, so the loads are independent of each other (no chain).
// Thread t owns the float4 column groups t and t + 256 (D <= 2048).  Every index is formed from r < R and a clamped id.
__global__ __launch_bounds__(256) void scatter_embed_ordered_kernel(const float* __restrict__ src, const int64_t* __restrict__ ids,
                                                                    float* __restrict__ demb, int64_t R, int D, int64_t V,
                                                                    int64_t padding_idx, float scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = blockIdx.x;
  const int64_t raw = ids[r];
  if (raw == padding_idx) return;                         // (block-uniform)
  const int64_t id = clamp_id(raw, V);
  __shared__ int found[4];
  bool f = false;
  for (int64_t base = (int64_t)wave * 64; base < r && !f; base += 256) {
    const int64_t q = base + lane;
    bool m = false;
    if (q < r) { const int64_t x = ids[q]; m = x != padding_idx && clamp_id(x, V) == id; }
    f = __ballot(m) != 0ull;
  }
  if (lane == 0) found[wave] = f ? 1 : 0;
  __syncthreads();
  if (found[0] | found[1] | found[2] | found[3]) return;  // not the first row of its id
  const int nquad = D >> 2;
  const f32x4* s4 = (const f32x4*)src;
  const int q0 = threadIdx.x, q1 = threadIdx.x + 256;
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
  if (q0 < nquad) a0 = s4[(size_t)r * nquad + q0];        // the sum starts from the first contribution
  if (q1 < nquad) a1 = s4[(size_t)r * nquad + q1];
  for (int64_t base = r + 1; base < R; base += 256) {
    uint64_t mask[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t q = base + 64 * u + lane;
      bool m = false;
      if (q < R) { const int64_t x = ids[q]; m = x != padding_idx && clamp_id(x, V) == id; }
      mask[u] = __ballot(m);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      uint64_t mk = mask[u];
      while (mk) {
        const int b = __ffsll((unsigned long long)mk) - 1;
        mk &= mk - 1;
        const size_t row = (size_t)(base + 64 * u + b);
        if (q0 < nquad) a0 += s4[row * nquad + q0];
        if (q1 < nquad) a1 += s4[row * nquad + q1];
      }
    }
  }
  f32x4* d4 = (f32x4*)demb;
  if (q0 < nquad) { const f32x4 p = a0 * scale; d4[(size_t)id * nquad + q0] = d4[(size_t)id * nquad + q0] + p; }
  if (q1 < nquad) { const f32x4 p = a1 * scale; d4[(size_t)id * nquad + q1] = d4[(size_t)id * nquad + q1] + p; }
}

// one thread per (position t, float4 column group): rows t, t + T, t + 2T, ... in ascending order
__global__ __launch_bounds__(256) void scatter_pos_ordered_kernel(const float* __restrict__ src, float* __restrict__ dpos, int64_t R,
                                                                  int64_t T, int D, int64_t pos_offset) {
  const int nquad = D >> 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nt = T < R ? T : R;
  if (i >= nt * nquad) return;
  const int64_t t = i / nquad;
  const int q = (int)(i - t * nquad);
  const f32x4* s4 = (const f32x4*)src;
  f32x4 a = s4[(size_t)t * nquad + q];
  for (int64_t r = t + T; r < R; r += T) a += s4[(size_t)r * nquad + q];
  f32x4* d4 = (f32x4*)dpos;
  const size_t o = (size_t)(t + pos_offset) * nquad + q;
  d4[o] = d4[o] + a;
}

// one block: strand t adds src[t], src[t + 256], ... ; thread 0 then adds the 256 strand sums in ascending order
__global__ __launch_bounds__(256) void sum_ordered_kernel(const float* __restrict__ src, int64_t n, float* __restrict__ dst) {
  __shared__ float red[SUM_STRANDS];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += SUM_STRANDS) s += src[i];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < SUM_STRANDS; ++i) t += red[i];
    dst[0] = t;
  }
}

// one wave per row.  Plain loss: lse - z_t.  Label smoothing adds eps (z_t - mean_j z_j), the mean from the per-tile logit sums
// (lane l adds tiles l, l + 64, ... in ascending order, then the wave's xor butterfly: a fixed order).
__global__ __launch_bounds__(256) void lmhead_row_loss_kernel(const float* __restrict__ row_lse, const float* __restrict__ tl,
                                                              const int64_t* __restrict__ targets, const float* __restrict__ part_sum,
                                                              float* __restrict__ row_loss, int R, int tiles, int64_t ignore, float eps,
                                                              float inv_v) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  if (r >= R) return;
  float l = 0.f;
  if (targets[r] != ignore) {                      // (wave-uniform)
    l = row_lse[r] - tl[r];
    if (part_sum) {
      float zs = 0.f;
      for (int t = lane; t < tiles; t += 64) zs += part_sum[(size_t)r * tiles + t];
      const float mean = wave_sum(zs) * inv_v;
      const float term = eps * (tl[r] - mean);
      l = l + term;
    }
  }
  if (lane == 0) row_loss[r] = l;
}

}  // namespace

extern "C" int vacnic_fold_ordered(const float* partials, int64_t ld, float* dst, float* dst2, int64_t NB, int64_t cols, void* stream) {
  VPLAN_REC(vacnic_fold_ordered, partials, ld, dst, dst2, NB, cols, stream);
  VCHECK(dst && cols > 0 && NB >= 0 && cols <= (1 << 24) && NB <= (1 << 24), VACNIC_BAD_SHAPE, "fold_ordered: dst is null, or NB / cols out of range");
  VCHECK(ld >= cols * (dst2 ? 2 : 1), VACNIC_BAD_SHAPE, "fold_ordered: ld=%ld is shorter than the %ld columns of a row", (long)ld,
         (long)(cols * (dst2 ? 2 : 1)));
  if (NB == 0) return VACNIC_OK;
  VCHECK(partials, VACNIC_BAD_SHAPE, "fold_ordered: null partials");
  hipLaunchKernelGGL(fold_ordered_kernel, dim3((unsigned)((cols + 63) / 64), dst2 ? 2 : 1), dim3(256), 0, (hipStream_t)stream, partials, ld,
                     dst, dst2, (int)NB, (int)cols);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int64_t vacnic_bias_grad_ordered_rows(int64_t M) {
  int64_t rb = (M + 63) / 64;
  if (rb > BIAS_MAX_ROW_BLOCKS) rb = BIAS_MAX_ROW_BLOCKS;
  return rb < 1 ? 1 : rb;
}

extern "C" int vacnic_bias_grad_ordered(const void* dy, float* dbias, int64_t M, int64_t N, int64_t ldy, float* partials,
                                        int64_t partial_rows, void* stream) {
  VPLAN_REC(vacnic_bias_grad_ordered, dy, dbias, M, N, ldy, partials, partial_rows, stream);
  VCHECK(dy && dbias && partials, VACNIC_BAD_SHAPE, "bias_grad_ordered: null operand");
  VCHECK(M >= 0 && N >= 0 && N <= (1 << 24) && ldy >= N, VACNIC_BAD_SHAPE, "bias_grad_ordered: bad shape M=%ld N=%ld ldy=%ld", (long)M, (long)N, (long)ldy);
  VCHECK((ldy & 7) == 0 && aligned16(dy), VACNIC_MISALIGNED, "bias_grad_ordered: dy rows must be 16-byte aligned");
  if (M == 0 || N == 0) return VACNIC_OK;
  const int64_t rb = vacnic_bias_grad_ordered_rows(M);
  VCHECK(partial_rows >= rb, VACNIC_BAD_SHAPE, "bias_grad_ordered: partials holds %ld rows, %ld needed (vacnic_bias_grad_ordered_rows)",
         (long)partial_rows, (long)rb);
  const int rows_per_block = (int)((M + rb - 1) / rb);
  hipLaunchKernelGGL(bias_partial_kernel, dim3((unsigned)((N + 511) / 512), (unsigned)rb), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)dy, partials, (long)M, (int)N, (long)ldy, rows_per_block);
  VLAUNCH_CHECK();
  // (a block of rows past the end — ceil(M / rows_per_block) < rb — has written zeros: r1 <= r0)
  return vacnic_fold_ordered(partials, N, dbias, nullptr, rb, N, stream);
}

extern "C" int vacnic_scatter_ordered(const float* src, const int64_t* ids, float* dembed, float* dpos, int64_t R, int64_t T, int64_t D,
                                      int64_t V, int64_t pos_offset, int64_t padding_idx, float scale, void* stream) {
  VPLAN_REC(vacnic_scatter_ordered, src, ids, dembed, dpos, R, T, D, V, pos_offset, padding_idx, scale, stream);
  VCHECK(src && (ids || !dembed), VACNIC_BAD_SHAPE, "scatter_ordered: null operand");
  VCHECK(R >= 0 && R < (1ll << 31) && T > 0 && D > 0 && D <= 2048 && (D & 3) == 0 && (V > 0 || !dembed) && pos_offset >= 0, VACNIC_BAD_SHAPE,
         "scatter_ordered: bad shape R=%ld T=%ld D=%ld V=%ld pos_offset=%ld (D a multiple of 4, <= 2048)", (long)R, (long)T, (long)D, (long)V,
         (long)pos_offset);
  VCHECK(aligned16(src) && aligned16(dembed) && aligned16(dpos), VACNIC_MISALIGNED, "scatter_ordered: pointers must be 16-byte aligned");
  if (R == 0) return VACNIC_OK;
  if (dembed) {
    hipLaunchKernelGGL(scatter_embed_ordered_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, src, ids, dembed, R, (int)D, V,
                       padding_idx, scale);
    VLAUNCH_CHECK();
  }
  if (dpos) {
    const int64_t n = (T < R ? T : R) * (D >> 2);
    hipLaunchKernelGGL(scatter_pos_ordered_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dpos, R, T, (int)D,
                       pos_offset);
    VLAUNCH_CHECK();
  }
  return VACNIC_OK;
}

extern "C" int vacnic_sum_ordered(const float* src, int64_t n, float* dst, void* stream) {
  VPLAN_REC(vacnic_sum_ordered, src, n, dst, stream);
  VCHECK(dst && n >= 0 && (src || n == 0), VACNIC_BAD_SHAPE, "sum_ordered: null operand");
  hipLaunchKernelGGL(sum_ordered_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, src, n, dst);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int vacnic_lmhead_row_loss(const float* row_lse, const float* tl, const int64_t* targets, const float* part_sum, int64_t R,
                                      int64_t V, int64_t part_tiles, int64_t ignore_index, float label_smoothing, float* row_loss,
                                      void* stream) {
  VPLAN_REC(vacnic_lmhead_row_loss, row_lse, tl, targets, part_sum, R, V, part_tiles, ignore_index, label_smoothing, row_loss, stream);
  VCHECK(row_lse && tl && targets && row_loss, VACNIC_BAD_SHAPE, "lmhead_row_loss: null operand");
  VCHECK(R > 0 && R < (1ll << 31) && V > 0, VACNIC_BAD_SHAPE, "lmhead_row_loss: empty problem");
  VCHECK(label_smoothing >= 0.f && label_smoothing < 1.f, VACNIC_BAD_SHAPE, "lmhead_row_loss: label_smoothing %g outside [0, 1)", (double)label_smoothing);
  const bool smooth = label_smoothing > 0.f;
  VCHECK(!smooth || (part_sum && part_tiles == (V + 255) / 256), VACNIC_BAD_SHAPE,
         "lmhead_row_loss: label_smoothing > 0 needs part_sum [R][ceil(V / 256)] of vacnic_lmhead_ce_fwd");
  hipLaunchKernelGGL(lmhead_row_loss_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, row_lse, tl, targets,
                     smooth ? part_sum : nullptr, row_loss, (int)R, (int)part_tiles, ignore_index, label_smoothing, 1.f / (float)V);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}
