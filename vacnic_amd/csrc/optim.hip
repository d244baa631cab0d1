// Fused AdamW over one flat fp32 arena + LR schedule on device (gfx950, HBM-bound: 16 B/param read,
// 14 B/param written).  Replaces torch.optim.AdamW's per-tensor loop (TRAIN:91,372-374) and
// get_linear_schedule_with_warmup (TRAIN:99-107).  lr/step live in device memory so the whole
// step is hipGraph-capturable.
#include "common.h"
#include <cstdlib>

namespace {

// hyper[0] = lr for this step, hyper[1] = step count t (float, 1-based after the increment)
__global__ void lr_step_kernel(float* hyper, float base_lr, float warmup, float total, unsigned long long* rng_counter) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (rng_counter) *rng_counter += 1ull;
    const float k = hyper[1];                 // optimizer steps taken so far == LambdaLR's current_step
    float lam;
    if (k < warmup) lam = k / fmaxf(1.f, warmup);
    else lam = fmaxf(0.f, (total - k) / fmaxf(1.f, total - warmup));
    hyper[0] = base_lr * lam;
    hyper[1] = k + 1.f;
  }
}

// A step that vacnic_grad_guard dropped: p, m, v and the shadow stay as they are (no weight decay either); the gradient is still
// cleared, or its NaNs would be accumulated into the next step.  *skip is the same for every thread of the launch.
__device__ __forceinline__ void skipped_step(float* __restrict__ g, long n4, int zero_grad) {
  if (!zero_grad) return;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) ((f32x4*)g)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

template <int UNR>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, bf16_t* __restrict__ pb,
                                                    const float* __restrict__ hyper, long n4, float b1, float b2,
                                                    float eps, float wd, float gscale, int zero_grad,
                                                    const float* __restrict__ clip, const int64_t* __restrict__ skip) {
  if (skip && *skip) { skipped_step(g, n4, zero_grad); return; }       // grad_guard's verdict: one uniform branch
  const float lr = hyper[0], t = hyper[1];
  if (clip) gscale *= clip[0];                  // clip_grad_norm_'s coefficient, computed on device by grad_clip_coef
  const float bc1 = 1.f - powf(b1, t), bc2 = 1.f - powf(b2, t);
  const float step_size = lr / bc1, inv_sqrt_bc2 = rsqrtf(bc2), decay = 1.f - lr * wd;
  const long stride = (long)gridDim.x * blockDim.x;
  // Launch shape (profiles/r1_adamw_microbench.txt): ALONE on the GPU this pass is fastest with one 4-wave workgroup per CU
  // (256 workgroups: 6.2 TB/s; 2048: 4.6; 65536: 5.0 on a 440M-parameter arena) — but in the training step it shares the GPU
  // with the next step's frozen-tower graphs, where a 256-workgroup launch loses its share of CUs and bandwidth (step 74.0 ms vs
  // 71.1 ms).  It sits on the critical path, so the launch is wide (65536 workgroups: 70.9 ms).  UNR (loads in flight per
  // stream per lane) made no difference at 1, 2, 4.
  for (long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x; i0 < n4; i0 += stride * UNR) {
    f32x4 pv[UNR], gv[UNR], mv[UNR], vv[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const long i = i0 + u * stride;
      if (i < n4) { pv[u] = ((f32x4*)p)[i]; gv[u] = ((f32x4*)g)[i]; mv[u] = ((f32x4*)m)[i]; vv[u] = ((f32x4*)v)[i]; }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const long i = i0 + u * stride;
      if (i >= n4) break;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gr = gv[u][e] * gscale;
        float pe = pv[u][e] * decay;
        const float me = b1 * mv[u][e] + (1.f - b1) * gr;
        const float ve = b2 * vv[u][e] + (1.f - b2) * gr * gr;
        pe -= step_size * me / (sqrtf(ve) * inv_sqrt_bc2 + eps);
        pv[u][e] = pe; mv[u][e] = me; vv[u][e] = ve;
      }
      ((f32x4*)p)[i] = pv[u]; ((f32x4*)m)[i] = mv[u]; ((f32x4*)v)[i] = vv[u];
      if (zero_grad) ((f32x4*)g)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (pb) ((u32x2*)pb)[i] = (u32x2){pack2bf(pv[u][0], pv[u][1]), pack2bf(pv[u][2], pv[u][3])};
    }
  }
}

// clip_grad_norm_ (TRAIN:365-366), pass 1: fixed-grid partial sums of (g*gscale)^2 — fixed grid + fixed
// per-thread order + a fixed-shape tree, so the norm is bit-reproducible run to run (no float atomics).
constexpr int kNormBlocks = 1024;
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long n4, float gscale,
                                                         float* __restrict__ partials) {
  float acc = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 gv = ((const f32x4*)g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float x = gv[e] * gscale; acc = fmaf(x, x, acc); }
  }
  __shared__ float red[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// pass 2 (one workgroup): out[0] = min(1, max_norm / (||g|| + 1e-6)), out[1] = ||g||   (torch.nn.utils.clip_grad_norm_)
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(const float* __restrict__ partials, int nparts, float max_norm,
                                                             float* __restrict__ out) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += partials[i];
  __shared__ float red[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float norm = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
    out[0] = fminf(1.f, max_norm / (norm + 1e-6f));
    out[1] = norm;
  }
}

// ---- parameter groups: per-segment lr multiple / weight decay / frozen flag (include/vacnic_hip.h) ---------------------------
// Lookup: a thread's 4-vector starts at absolute arena element `a`; first_seg[a >> 10] is the segment holding the first element
// of that 1024-element block, and the thread walks seg_start forward from there — a few entries at most for a table built from
// parameters (a block of 1024 elements holds few of them), all of it hits in L2 (the table is < 0.1 % of the streamed bytes).
struct GroupTable {
  const int64_t* __restrict__ seg_start; const vacnic_adamw_seg* __restrict__ seg; const int32_t* __restrict__ first_seg;
  long nseg, nblocks, elem_base;
};
// segment of absolute element a; clamped, so a malformed table cannot index outside itself
__device__ __forceinline__ long seg_of(const GroupTable& t, long a) {
  long b = a >> 10;
  b = b < 0 ? 0 : (b >= t.nblocks ? t.nblocks - 1 : b);
  long s = t.first_seg[b];
  s = s < 0 ? 0 : (s >= t.nseg ? t.nseg - 1 : s);
  while (s < t.nseg - 1 && t.seg_start[s + 1] <= a) ++s;
  return s;
}
// first element after segment s (the last segment extends to the end of whatever range is being processed)
__device__ __forceinline__ long seg_end(const GroupTable& t, long s) { return s < t.nseg - 1 ? t.seg_start[s + 1] : INT64_MAX; }

// adamw_kernel's per-element arithmetic with the multiply-adds it compiles to written out (the compiler is free to contract
// a * b + c * d either way round; a one-segment table must reproduce adamw_kernel bit for bit, which the tests check):
//   m = fma(b1, m, (1 - b1) g);  v = fma(b2, v, ((1 - b2) g) g);  p = fma(decay, p, -(step_size m / fma(sqrt(v), 1/sqrt(bc2), eps)))
//   decay = fma(-lr, wd, 1)
__device__ __forceinline__ float adam_m(float b1, float m, float gr) { return fmaf(b1, m, (1.f - b1) * gr); }
__device__ __forceinline__ float adam_v(float b2, float v, float gr) { return fmaf(b2, v, (1.f - b2) * gr * gr); }
__device__ __forceinline__ float adam_p(float p, float decay, float step_size, float me, float ve, float inv_sqrt_bc2, float eps) {
  return fmaf(decay, p, -(step_size * me / fmaf(sqrtf(ve), inv_sqrt_bc2, eps)));
}

__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, bf16_t* __restrict__ pb,
                                                           const float* __restrict__ hyper, long n4, float b1, float b2, float eps,
                                                           float gscale, int zero_grad, const float* __restrict__ clip,
                                                           GroupTable tab, const int64_t* __restrict__ skip) {
  if (skip && *skip) { skipped_step(g, n4, zero_grad); return; }
  const float lr0 = hyper[0], t = hyper[1];
  if (clip) gscale *= clip[0];
  const float bc1 = 1.f - powf(b1, t), bc2 = 1.f - powf(b2, t);
  const float inv_sqrt_bc2 = rsqrtf(bc2);
  const long stride = (long)gridDim.x * blockDim.x;
  // launch shape and per-element arithmetic of adamw_kernel<1>: one segment {1, wd, not frozen} reproduces it bit for bit
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 pv = ((f32x4*)p)[i], gv = ((f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
    const long a = tab.elem_base + (i << 2);
    long s = seg_of(tab, a);
    vacnic_adamw_seg sg = tab.seg[s];
    if (a + 4 <= seg_end(tab, s)) {                     // the whole vector lies in one segment (all but a few vectors per boundary)
      if (!sg.frozen) {
        const float lr = lr0 * sg.lr_scale;
        const float step_size = lr / bc1, decay = fmaf(-lr, sg.weight_decay, 1.f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float gr = gv[e] * gscale;
          const float me = adam_m(b1, mv[e], gr), ve = adam_v(b2, vv[e], gr);
          pv[e] = adam_p(pv[e], decay, step_size, me, ve, inv_sqrt_bc2, eps); mv[e] = me; vv[e] = ve;
        }
        ((f32x4*)p)[i] = pv; ((f32x4*)m)[i] = mv; ((f32x4*)v)[i] = vv;
        if (pb) ((u32x2*)pb)[i] = (u32x2){pack2bf(pv[0], pv[1]), pack2bf(pv[2], pv[3])};
      }
    } else {                                            // a boundary inside the vector: element by element, scalar stores
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (a + e >= seg_end(tab, s)) { s = seg_of(tab, a + e); sg = tab.seg[s]; }
        if (sg.frozen) continue;
        const float lr = lr0 * sg.lr_scale;
        const float step_size = lr / bc1, decay = fmaf(-lr, sg.weight_decay, 1.f);
        const float gr = gv[e] * gscale;
        const float me = adam_m(b1, mv[e], gr), ve = adam_v(b2, vv[e], gr);
        const float pe = adam_p(pv[e], decay, step_size, me, ve, inv_sqrt_bc2, eps);
        const long j = (i << 2) + e;
        p[j] = pe; m[j] = me; v[j] = ve;
        if (pb) pb[j] = f2bf(pe);
      }
    }
    if (zero_grad) ((f32x4*)g)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};       // frozen elements too: backward still accumulates into them
  }
}

// ---- AdamW + exponential moving average of the weights (vacnic_adamw_ema, include/vacnic_hip.h) ------------------------------
// The loop of adamw_groups_kernel with one more fp32 stream: the new p is in registers, so the average costs 4 B read + 4 B
// written per parameter (a separate pass: 12 B and a launch).  GROUPED = false is the one-group case without the table lookup:
// lr = hyper[0] and the struct's weight decay, which adamw_kernel<1> computes bit for bit (see adam_m / adam_v / adam_p).
struct EmaArgs { float* __restrict__ ema; float decay; int warmup; };
// this step's decay: torch_ema / timm warm-up over Adam's own step count t (>= 1 once vacnic_lr_step has run)
__device__ __forceinline__ float ema_decay_at(const EmaArgs& e, float t) {
  return e.warmup ? fminf(e.decay, (1.f + t) / (10.f + t)) : e.decay;
}
template <bool GROUPED>
__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, bf16_t* __restrict__ pb,
                                                        const float* __restrict__ hyper, long n4, float b1, float b2, float eps,
                                                        float wd, float gscale, int zero_grad, const float* __restrict__ clip,
                                                        GroupTable tab, const int64_t* __restrict__ skip, EmaArgs ea) {
  if (skip && *skip) { skipped_step(g, n4, zero_grad); return; }      // a dropped step: the average stays too
  const float lr0 = hyper[0], t = hyper[1];
  if (clip) gscale *= clip[0];
  const float bc1 = 1.f - powf(b1, t), bc2 = 1.f - powf(b2, t);
  const float inv_sqrt_bc2 = rsqrtf(bc2);
  const float d = ema_decay_at(ea, t), omd = 1.f - d;
  float* __restrict__ ema = ea.ema;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 pv = ((f32x4*)p)[i], gv = ((f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
    f32x4 ev = ((f32x4*)ema)[i];                          // with the other four streams, ahead of the table lookup
    const long a = tab.elem_base + (i << 2);
    long s = 0;
    vacnic_adamw_seg sg = {1.f, wd, 0, 0};
    bool whole = true;
    if (GROUPED) {
      s = seg_of(tab, a);
      sg = tab.seg[s];
      whole = a + 4 <= seg_end(tab, s);
    }
    if (whole) {                                          // the whole vector lies in one segment
      if (!sg.frozen) {
        const float lr = GROUPED ? lr0 * sg.lr_scale : lr0;
        const float step_size = lr / bc1, decay = fmaf(-lr, sg.weight_decay, 1.f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float gr = gv[e] * gscale;
          const float me = adam_m(b1, mv[e], gr), ve = adam_v(b2, vv[e], gr);
          pv[e] = adam_p(pv[e], decay, step_size, me, ve, inv_sqrt_bc2, eps); mv[e] = me; vv[e] = ve;
          ev[e] = fmaf(d, ev[e], omd * pv[e]);
        }
        ((f32x4*)p)[i] = pv; ((f32x4*)m)[i] = mv; ((f32x4*)v)[i] = vv; ((f32x4*)ema)[i] = ev;
        if (pb) ((u32x2*)pb)[i] = (u32x2){pack2bf(pv[0], pv[1]), pack2bf(pv[2], pv[3])};
      }
    } else {                                              // a boundary inside the vector: element by element
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (a + e >= seg_end(tab, s)) { s = seg_of(tab, a + e); sg = tab.seg[s]; }
        if (sg.frozen) continue;
        const float lr = lr0 * sg.lr_scale;
        const float step_size = lr / bc1, decay = fmaf(-lr, sg.weight_decay, 1.f);
        const float gr = gv[e] * gscale;
        const float me = adam_m(b1, mv[e], gr), ve = adam_v(b2, vv[e], gr);
        const float pe = adam_p(pv[e], decay, step_size, me, ve, inv_sqrt_bc2, eps);
        const long j = (i << 2) + e;
        p[j] = pe; m[j] = me; v[j] = ve;
        ema[j] = fmaf(d, ev[e], omd * pe);
        if (pb) pb[j] = f2bf(pe);
      }
    }
    if (zero_grad) ((f32x4*)g)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
}

// p <-> ema by contents, shadow = bf16(new p) with cast_f32_bf16_kernel's rounding (pack2bf)
__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ ema, bf16_t* __restrict__ pb, long n4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 pv = ((f32x4*)p)[i], ev = ((f32x4*)ema)[i];
    ((f32x4*)p)[i] = ev; ((f32x4*)ema)[i] = pv;
    if (pb) ((u32x2*)pb)[i] = (u32x2){pack2bf(ev[0], ev[1]), pack2bf(ev[2], ev[3])};
  }
}

// grad_sumsq_kernel over the non-frozen elements: same grid, same per-thread order, same tree
__global__ __launch_bounds__(256) void grad_sumsq_groups_kernel(const float* __restrict__ g, long n4, float gscale,
                                                                float* __restrict__ partials, GroupTable tab) {
  float acc = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 gv = ((const f32x4*)g)[i];
    const long a = tab.elem_base + (i << 2);
    long s = seg_of(tab, a);
    int frozen = tab.seg[s].frozen;
    if (a + 4 <= seg_end(tab, s)) {
      if (!frozen) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float x = gv[e] * gscale; acc = fmaf(x, x, acc); }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (a + e >= seg_end(tab, s)) { s = seg_of(tab, a + e); frozen = tab.seg[s].frozen; }
        if (!frozen) { const float x = gv[e] * gscale; acc = fmaf(x, x, acc); }
      }
    }
  }
  __shared__ float red[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- non-finite gradient guard (vacnic_grad_guard, include/vacnic_hip.h) -----------------------------------------------------
// Pass 1 = grad_sumsq_kernel / grad_sumsq_groups_kernel (same grid, same per-thread order, same tree: the partial sums are theirs
// bit for bit) that also keeps, per block, the smallest absolute element index whose scaled gradient has a non-finite square.
__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ long wave_min_i64(long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const long w = __shfl_xor((long long)v, o, 64); v = w < v ? w : v; }
  return v;
}
// block reduction of the (sum, smallest index) pair, the clip-norm kernels' tree for the sum; the result is thread 0's
__device__ __forceinline__ void guard_block_reduce(float& acc, long& first) {
  __shared__ float red[4];
  __shared__ long redi[4];
  acc = wave_sum(acc);
  first = wave_min_i64(first);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = acc; redi[threadIdx.x >> 6] = first; }
  __syncthreads();
  if (threadIdx.x == 0) {
    acc = (red[0] + red[1]) + (red[2] + red[3]);
    const long a = redi[0] < redi[1] ? redi[0] : redi[1], b = redi[2] < redi[3] ? redi[2] : redi[3];
    first = a < b ? a : b;
  }
}
__global__ __launch_bounds__(256) void grad_guard_sumsq_kernel(const float* __restrict__ g, long n4, float gscale, long elem_base,
                                                               float* __restrict__ partials, int64_t* __restrict__ first_idx) {
  float acc = 0.f;
  long first = INT64_MAX;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 gv = ((const f32x4*)g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = gv[e] * gscale;
      acc = fmaf(x, x, acc);
      const long a = elem_base + (i << 2) + e;              // i rises and e rises: the first hit of a thread is its smallest
      if (nonfinite(x * x) && a < first) first = a;
    }
  }
  guard_block_reduce(acc, first);
  if (threadIdx.x == 0) { partials[blockIdx.x] = acc; first_idx[blockIdx.x] = first; }
}
__global__ __launch_bounds__(256) void grad_guard_sumsq_groups_kernel(const float* __restrict__ g, long n4, float gscale,
                                                                      float* __restrict__ partials, int64_t* __restrict__ first_idx,
                                                                      GroupTable tab) {
  float acc = 0.f;
  long first = INT64_MAX;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 gv = ((const f32x4*)g)[i];
    const long a = tab.elem_base + (i << 2);
    long s = seg_of(tab, a);
    int frozen = tab.seg[s].frozen;
    if (a + 4 <= seg_end(tab, s)) {
      if (!frozen) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = gv[e] * gscale;
          acc = fmaf(x, x, acc);
          if (nonfinite(x * x) && a + e < first) first = a + e;
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (a + e >= seg_end(tab, s)) { s = seg_of(tab, a + e); frozen = tab.seg[s].frozen; }
        if (!frozen) {
          const float x = gv[e] * gscale;
          acc = fmaf(x, x, acc);
          if (nonfinite(x * x) && a + e < first) first = a + e;
        }
      }
    }
  }
  guard_block_reduce(acc, first);
  if (threadIdx.x == 0) { partials[blockIdx.x] = acc; first_idx[blockIdx.x] = first; }
}
// Pass 2 (one workgroup): grad_clip_coef_kernel's sum and coefficient, the verdict, the counters, and on a skip the undo of
// lr_step's increment of hyper[1].  skip <=> the sum of squares is not finite: squares cannot cancel, so that holds exactly when
// some element's square is non-finite or the fp32 sum itself overflowed (then no element is to blame: index -1).
__global__ __launch_bounds__(256) void grad_guard_verdict_kernel(const float* __restrict__ partials,
                                                                 const int64_t* __restrict__ first_idx, int nparts, float max_norm,
                                                                 float* __restrict__ out, int64_t* __restrict__ state,
                                                                 float* __restrict__ hyper) {
  float acc = 0.f;
  long first = INT64_MAX;
  for (int i = threadIdx.x; i < nparts; i += 256) {
    acc += partials[i];
    const long f = first_idx[i];
    first = f < first ? f : first;
  }
  guard_block_reduce(acc, first);
  if (threadIdx.x == 0) {
    const float sumsq = acc;
    const float norm = sqrtf(sumsq);
    out[0] = max_norm > 0.f ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;
    out[1] = norm;
    const long f = first;
    if (nonfinite(sumsq)) {
      state[0] = 1; state[1] += 1; state[2] += 1;
      state[3] = f == INT64_MAX ? -1 : f;
      hyper[1] -= 1.f;                       // neither Adam's t nor the schedule position advances on a dropped step
    } else {
      state[0] = 0; state[2] = 0;
    }
  }
}

__global__ __launch_bounds__(256) void cast_f32_bf16_kernel(const float* __restrict__ s, bf16_t* __restrict__ d, long n) {
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 v = ((const f32x4*)s)[i];
    ((u32x2*)d)[i] = (u32x2){pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
  }
  if (blockIdx.x == 0)
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += blockDim.x) d[i] = f2bf(s[i]);
}
__global__ __launch_bounds__(256) void cast_bf16_f32_kernel(const bf16_t* __restrict__ s, float* __restrict__ d, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) d[i] = bf2f(s[i]);
}

inline unsigned grid_for(long work) {
  long b = (work + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

}  // namespace

extern "C" int vacnic_lr_step(float* hyper, float base_lr, float warmup_steps, float total_steps, uint64_t* rng_counter, void* stream) {
  VPLAN_REC(vacnic_lr_step, hyper, base_lr, warmup_steps, total_steps, rng_counter, stream);
  VCHECK(hyper, VACNIC_BAD_SHAPE, "lr_step: null hyper");
  hipLaunchKernelGGL(lr_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hyper, base_lr, warmup_steps, total_steps, (unsigned long long*)rng_counter);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int vacnic_adamw(const vacnic_adamw_args* a, void* stream) {
  VPLAN_REC_STRUCT(vacnic_adamw, a, stream);
  VCHECK(a && a->p && a->g && a->m && a->v && a->hyper, VACNIC_BAD_SHAPE, "adamw: null operand");
  VCHECK((a->n & 3) == 0, VACNIC_BAD_SHAPE, "adamw: n=%ld must be a multiple of 4 (pad the arena)", (long)a->n);
  VCHECK(aligned16(a->p) && aligned16(a->g) && aligned16(a->m) && aligned16(a->v) && (!a->p_bf16 || (((uintptr_t)a->p_bf16) & 7) == 0),
         VACNIC_MISALIGNED, "adamw: arenas must be 16-byte aligned");
  if (a->n == 0) return VACNIC_OK;
  const long n4 = a->n >> 2;
  unsigned blocks = 65536;                     // wide launch (see the kernel comment); small arenas: one element per thread
  const long need = (n4 + 255) / 256;
  if (need < blocks) blocks = (unsigned)(need < 1 ? 1 : need);
  hipLaunchKernelGGL(adamw_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a->p, a->g, a->m, a->v,
                     (bf16_t*)a->p_bf16, a->hyper, n4, a->beta1, a->beta2, a->eps, a->weight_decay, a->grad_scale, a->zero_grad,
                     a->clip_coef, a->skip);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int vacnic_grad_clip_coef(const float* g, int64_t n, float grad_scale, float max_norm, float* partials,
                                     float* out, void* stream) {
  VPLAN_REC(vacnic_grad_clip_coef, g, n, grad_scale, max_norm, partials, out, stream);
  VCHECK(g && partials && out, VACNIC_BAD_SHAPE, "grad_clip_coef: null operand");
  VCHECK((n & 3) == 0 && aligned16(g), VACNIC_BAD_SHAPE, "grad_clip_coef: arena must be 16-byte aligned, n=%ld a multiple of 4", (long)n);
  VCHECK(max_norm > 0.f, VACNIC_BAD_SHAPE, "grad_clip_coef: max_norm must be > 0");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(kNormBlocks), dim3(256), 0, (hipStream_t)stream, g, (long)(n >> 2), grad_scale, partials);
  VLAUNCH_CHECK();
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, kNormBlocks, max_norm, out);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

// ordering and coverage of the table are the host builder's to check (it lives in device memory: reading it here would sync)
#define VCHECK_GROUP_TABLE(a, what)                                                                                              \
  VCHECK((a)->seg_start && (a)->seg && (a)->first_seg, VACNIC_BAD_SHAPE, what ": null group table");                             \
  VCHECK((a)->nseg >= 1 && (a)->nblocks >= 1 && (a)->elem_base >= 0, VACNIC_BAD_SHAPE,                                           \
         what ": nseg=%ld and nblocks=%ld must be >= 1, elem_base=%ld >= 0", (long)(a)->nseg, (long)(a)->nblocks,                \
         (long)(a)->elem_base);                                                                                                  \
  VCHECK((a)->elem_base + (a)->n <= (a)->nblocks * 1024, VACNIC_BAD_SHAPE,                                                       \
         what ": elements [%ld, %ld) lie outside the table's %ld blocks of 1024", (long)(a)->elem_base,                          \
         (long)((a)->elem_base + (a)->n), (long)(a)->nblocks)

extern "C" int vacnic_adamw_groups(const vacnic_adamw_groups_args* a, void* stream) {
  VPLAN_REC_STRUCT(vacnic_adamw_groups, a, stream);
  VCHECK(a && a->p && a->g && a->m && a->v && a->hyper, VACNIC_BAD_SHAPE, "adamw_groups: null operand");
  VCHECK(a->n >= 0 && (a->n & 3) == 0, VACNIC_BAD_SHAPE, "adamw_groups: n=%ld must be a multiple of 4 (pad the arena)", (long)a->n);
  VCHECK(aligned16(a->p) && aligned16(a->g) && aligned16(a->m) && aligned16(a->v) && (!a->p_bf16 || (((uintptr_t)a->p_bf16) & 7) == 0),
         VACNIC_MISALIGNED, "adamw_groups: arenas must be 16-byte aligned");
  VCHECK_GROUP_TABLE(a, "adamw_groups");
  if (a->n == 0) return VACNIC_OK;
  const long n4 = a->n >> 2;
  unsigned blocks = 65536;                     // the launch shape of vacnic_adamw
  const long need = (n4 + 255) / 256;
  if (need < blocks) blocks = (unsigned)(need < 1 ? 1 : need);
  const GroupTable tab = {a->seg_start, a->seg, a->first_seg, (long)a->nseg, (long)a->nblocks, (long)a->elem_base};
  hipLaunchKernelGGL(adamw_groups_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a->p, a->g, a->m, a->v,
                     (bf16_t*)a->p_bf16, a->hyper, n4, a->beta1, a->beta2, a->eps, a->grad_scale, a->zero_grad, a->clip_coef, tab, a->skip);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int vacnic_adamw_ema(const vacnic_adamw_ema_args* a, void* stream) {
  VPLAN_REC_STRUCT(vacnic_adamw_ema, a, stream);
  VCHECK(a && a->p && a->g && a->m && a->v && a->hyper, VACNIC_BAD_SHAPE, "adamw_ema: null operand");
  VCHECK(a->ema, VACNIC_BAD_SHAPE, "adamw_ema: null ema");
  VCHECK(a->n >= 0 && (a->n & 3) == 0, VACNIC_BAD_SHAPE, "adamw_ema: n=%ld must be a multiple of 4 (pad the arena)", (long)a->n);
  VCHECK(a->ema_decay > 0.f && a->ema_decay < 1.f, VACNIC_BAD_SHAPE, "adamw_ema: ema_decay=%g must lie in (0, 1)", (double)a->ema_decay);
  VCHECK(aligned16(a->p) && aligned16(a->g) && aligned16(a->m) && aligned16(a->v) && aligned16(a->ema) &&
             (!a->p_bf16 || (((uintptr_t)a->p_bf16) & 7) == 0),
         VACNIC_MISALIGNED, "adamw_ema: arenas must be 16-byte aligned");
  const bool grouped = a->seg_start || a->seg || a->first_seg;
  if (grouped) {
    VCHECK_GROUP_TABLE(a, "adamw_ema");
  } else {
    VCHECK(a->elem_base >= 0, VACNIC_BAD_SHAPE, "adamw_ema: elem_base=%ld must be >= 0", (long)a->elem_base);
  }
  if (a->n == 0) return VACNIC_OK;
  const long n4 = a->n >> 2;
  unsigned blocks = 65536;                     // the launch shape of vacnic_adamw
  const long need = (n4 + 255) / 256;
  if (need < blocks) blocks = (unsigned)(need < 1 ? 1 : need);
  const GroupTable tab = {a->seg_start, a->seg, a->first_seg, (long)a->nseg, (long)a->nblocks, (long)a->elem_base};
  const EmaArgs ea = {a->ema, a->ema_decay, a->ema_warmup};
  if (grouped)
    hipLaunchKernelGGL(adamw_ema_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a->p, a->g, a->m, a->v,
                       (bf16_t*)a->p_bf16, a->hyper, n4, a->beta1, a->beta2, a->eps, a->weight_decay, a->grad_scale, a->zero_grad,
                       a->clip_coef, tab, a->skip, ea);
  else
    hipLaunchKernelGGL(adamw_ema_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a->p, a->g, a->m, a->v,
                       (bf16_t*)a->p_bf16, a->hyper, n4, a->beta1, a->beta2, a->eps, a->weight_decay, a->grad_scale, a->zero_grad,
                       a->clip_coef, tab, a->skip, ea);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int vacnic_ema_swap(float* p, float* ema, void* p_bf16, int64_t n, void* stream) {
  VPLAN_REC(vacnic_ema_swap, p, ema, p_bf16, n, stream);
  VCHECK(p && ema, VACNIC_BAD_SHAPE, "ema_swap: null operand");
  VCHECK(n >= 0 && (n & 3) == 0, VACNIC_BAD_SHAPE, "ema_swap: n=%ld must be a multiple of 4 (pad the arena)", (long)n);
  VCHECK(aligned16(p) && aligned16(ema) && (!p_bf16 || (((uintptr_t)p_bf16) & 7) == 0), VACNIC_MISALIGNED,
         "ema_swap: p and ema must be 16-byte aligned, the shadow 8-byte");
  VCHECK(p != ema, VACNIC_BAD_SHAPE, "ema_swap: p and ema are the same buffer");
  if (n == 0) return VACNIC_OK;
  hipLaunchKernelGGL(ema_swap_kernel, dim3(grid_for(n >> 2)), dim3(256), 0, (hipStream_t)stream, p, ema, (bf16_t*)p_bf16, (long)(n >> 2));
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int vacnic_grad_clip_coef_groups(const vacnic_grad_clip_groups_args* a, void* stream) {
  VPLAN_REC_STRUCT(vacnic_grad_clip_coef_groups, a, stream);
  VCHECK(a && a->g && a->partials && a->out, VACNIC_BAD_SHAPE, "grad_clip_coef_groups: null operand");
  VCHECK(a->n >= 0 && (a->n & 3) == 0 && aligned16(a->g), VACNIC_BAD_SHAPE,
         "grad_clip_coef_groups: arena must be 16-byte aligned, n=%ld a multiple of 4", (long)a->n);
  VCHECK(a->max_norm > 0.f, VACNIC_BAD_SHAPE, "grad_clip_coef_groups: max_norm must be > 0");
  VCHECK_GROUP_TABLE(a, "grad_clip_coef_groups");
  const GroupTable tab = {a->seg_start, a->seg, a->first_seg, (long)a->nseg, (long)a->nblocks, (long)a->elem_base};
  hipLaunchKernelGGL(grad_sumsq_groups_kernel, dim3(kNormBlocks), dim3(256), 0, (hipStream_t)stream, a->g, (long)(a->n >> 2),
                     a->grad_scale, a->partials, tab);
  VLAUNCH_CHECK();
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a->partials, kNormBlocks, a->max_norm, a->out);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int vacnic_grad_guard(const vacnic_grad_guard_args* a, void* stream) {
  VPLAN_REC_STRUCT(vacnic_grad_guard, a, stream);
  VCHECK(a && a->g && a->partials && a->first_idx && a->out && a->state && a->hyper, VACNIC_BAD_SHAPE, "grad_guard: null operand");
  VCHECK(a->n >= 0 && (a->n & 3) == 0 && aligned16(a->g), VACNIC_BAD_SHAPE,
         "grad_guard: arena must be 16-byte aligned, n=%ld a multiple of 4", (long)a->n);
  VCHECK(a->elem_base >= 0, VACNIC_BAD_SHAPE, "grad_guard: elem_base=%ld must be >= 0", (long)a->elem_base);
  VCHECK(((uintptr_t)a->first_idx & 7) == 0 && ((uintptr_t)a->state & 7) == 0, VACNIC_MISALIGNED, "grad_guard: first_idx and state must be 8-byte aligned");
  const bool grouped = a->seg_start || a->seg || a->first_seg;
  if (grouped) {
    VCHECK_GROUP_TABLE(a, "grad_guard");
    const GroupTable tab = {a->seg_start, a->seg, a->first_seg, (long)a->nseg, (long)a->nblocks, (long)a->elem_base};
    hipLaunchKernelGGL(grad_guard_sumsq_groups_kernel, dim3(kNormBlocks), dim3(256), 0, (hipStream_t)stream, a->g, (long)(a->n >> 2),
                       a->grad_scale, a->partials, a->first_idx, tab);
  } else {
    hipLaunchKernelGGL(grad_guard_sumsq_kernel, dim3(kNormBlocks), dim3(256), 0, (hipStream_t)stream, a->g, (long)(a->n >> 2),
                       a->grad_scale, (long)a->elem_base, a->partials, a->first_idx);
  }
  VLAUNCH_CHECK();
  hipLaunchKernelGGL(grad_guard_verdict_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a->partials, a->first_idx, kNormBlocks,
                     a->max_norm, a->out, a->state, a->hyper);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int vacnic_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream) {
  VPLAN_REC(vacnic_cast_f32_bf16, src, dst, n, stream);
  VCHECK(src && dst, VACNIC_BAD_SHAPE, "cast: null operand");
  VCHECK(aligned16(src) && (((uintptr_t)dst) & 7) == 0, VACNIC_MISALIGNED, "cast_f32_bf16: misaligned");
  if (n == 0) return VACNIC_OK;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(grid_for(n >> 2)), dim3(256), 0, (hipStream_t)stream, src, (bf16_t*)dst, (long)n);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}
extern "C" int vacnic_cast_bf16_f32(const void* src, float* dst, int64_t n, void* stream) {
  VPLAN_REC(vacnic_cast_bf16_f32, src, dst, n, stream);
  VCHECK(src && dst, VACNIC_BAD_SHAPE, "cast: null operand");
  if (n == 0) return VACNIC_OK;
  hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, dst, (long)n);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}
