// Fused AdamW over one flat fp32 arena + LR schedule on device (gfx950, HBM-bound: 16 B/param read,
// 14 B/param written).  Replaces torch.optim.AdamW's per-tensor loop (TRAIN:91,372-374) and
// get_linear_schedule_with_warmup (TRAIN:99-107).  lr/step live in device memory so the whole
// step is hipGraph-capturable.
#include "common.h"
#include <cstdlib>

namespace {

// hyper[0] = lr for this step, hyper[1] = step count t (float, 1-based after the increment)
__device__ __forceinline__ void advance_schedule(float* hyper, float base_lr, float warmup, float total) {
  const float k = hyper[1];                   // optimizer steps taken so far == LambdaLR's current_step
  float lam;
  if (k < warmup) lam = k / fmaxf(1.f, warmup);
  else lam = fmaxf(0.f, (total - k) / fmaxf(1.f, total - warmup));
  hyper[0] = base_lr * lam;
  hyper[1] = k + 1.f;
}
__global__ void lr_step_kernel(float* hyper, float base_lr, float warmup, float total, unsigned long long* rng_counter) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (rng_counter) *rng_counter += 1ull;
    advance_schedule(hyper, base_lr, warmup, total);
  }
}

// ---- gradient accumulation: k micro-batches per optimizer step (vacnic_lr_step_accum, include/vacnic_hip.h) -------------------
// The STEP WORD that AdamW, the statistics pass and the guard share: 0 apply, 1 dropped by the guard, 2 hold (a micro-batch that
// only adds to the gradient).  Every micro-batch issues the launches of a full step; on a hold each of them loads the word and
// leaves, so eager steps, launch plans and graphs need not know which kind of micro-batch they carry.
constexpr int64_t kHold = 2;
// accum = {step word, micro-batches pending, groups completed, 0}.  The dropout counter advances on every call (each micro-batch
// draws its own masks); hyper only when the group is complete, with lr_step_kernel's arithmetic.
__global__ void lr_step_accum_kernel(float* hyper, float base_lr, float warmup, float total, unsigned long long* rng_counter,
                                     int64_t* accum, int k) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (rng_counter) *rng_counter += 1ull;
    const int64_t pending = accum[1];
    if (pending + 1 < k) {
      accum[1] = pending + 1;
      accum[0] = kHold;
    } else {
      accum[1] = 0;
      accum[2] += 1;
      accum[0] = 0;
      advance_schedule(hyper, base_lr, warmup, total);
    }
  }
}

// A step that vacnic_grad_guard dropped: p, m, v and the shadow stay as they are (no weight decay either); the gradient is still
// cleared, or its NaNs would be accumulated into the next step.  *skip is the same for every thread of the launch.
__device__ __forceinline__ void skipped_step(float* __restrict__ g, long n4, int zero_grad) {
  if (!zero_grad) return;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) ((f32x4*)g)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// clip_grad_norm_ (TRAIN:365-366), pass 2 (one workgroup) over the partial sums of grad_sumsq_kernel below:
// out[0] = min(1, max_norm / (||g|| + 1e-6)), out[1] = ||g||
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(const float* __restrict__ partials, int nparts, float max_norm,
                                                             float* __restrict__ out, const int64_t* __restrict__ hold) {
  if (hold && *hold == kHold) return;           // a held micro-batch: pass 1 wrote no partial sums, out keeps the last group's pair
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

// The per-element arithmetic with every multiply-add written out, so that no instantiation depends on how the compiler contracts
// a * b + c * d (all entry points must agree bit for bit on what they share, which the tests check):
//   m = fma(b1, m, (1 - b1) g);  v = fma(b2, v, ((1 - b2) g) g);  p = fma(decay, p, -(step_size m / fma(sqrt(v), 1/sqrt(bc2), eps)))
//   decay = fma(-lr, wd, 1)
__device__ __forceinline__ float adam_m(float b1, float m, float gr) { return fmaf(b1, m, (1.f - b1) * gr); }
__device__ __forceinline__ float adam_v(float b2, float v, float gr) { return fmaf(b2, v, (1.f - b2) * gr * gr); }
__device__ __forceinline__ float adam_p(float p, float decay, float step_size, float me, float ve, float inv_sqrt_bc2, float eps) {
  return fmaf(decay, p, -(step_size * me / fmaf(sqrtf(ve), inv_sqrt_bc2, eps)));
}

// the moving average of the weights (vacnic_adamw_ema, include/vacnic_hip.h), laid out like p
struct EmaArgs { float* __restrict__ ema; float decay; int warmup; };
// this step's decay: torch_ema / timm warm-up over Adam's own step count t (>= 1 once vacnic_lr_step has run)
__device__ __forceinline__ float ema_decay_at(const EmaArgs& e, float t) {
  return e.warmup ? fminf(e.decay, (1.f + t) / (10.f + t)) : e.decay;
}

// The one AdamW loop, behind vacnic_adamw, vacnic_adamw_groups and vacnic_adamw_ema.
// GROUPED: lr multiple, weight decay and frozen flag come from the segment table; otherwise one group {1, wd, trained} and no lookup.
// EMA: one more fp32 stream; the new p is in registers, so the average costs 4 B read + 4 B written per parameter (a separate
// pass: 12 B and a launch).
// Launch shape (profiles/r1_adamw_microbench.txt): ALONE on the GPU this pass is fastest with one 4-wave workgroup per CU
// (256 workgroups: 6.2 TB/s; 2048: 4.6; 65536: 5.0 on a 440M-parameter arena) — but in the training step it shares the GPU
// with the next step's frozen-tower graphs, where a 256-workgroup launch loses its share of CUs and bandwidth (step 74.0 ms vs
// 71.1 ms).  It sits on the critical path, so the launch is wide (65536 workgroups: 70.9 ms).  More loads in flight per stream
// per lane (an unroll of 2 or 4 vectors) made no difference.
template <bool GROUPED, bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, bf16_t* __restrict__ pb,
                                                    const float* __restrict__ hyper, long n4, float b1, float b2, float eps,
                                                    float wd, float gscale, int zero_grad, const float* __restrict__ clip,
                                                    GroupTable tab, const int64_t* __restrict__ skip, EmaArgs ea) {
  if (skip) {                                   // the step word, one uniform branch on one loaded value
    const int64_t word = *skip;
    if (word == kHold) return;                  // a held micro-batch: nothing is read or written, the gradient keeps accumulating
    if (word) { skipped_step(g, n4, zero_grad); return; }             // grad_guard's verdict: the average stays too
  }
  const float lr0 = hyper[0], t = hyper[1];
  if (clip) gscale *= clip[0];                  // clip_grad_norm_'s coefficient, computed on device by grad_clip_coef
  const float bc1 = 1.f - powf(b1, t), bc2 = 1.f - powf(b2, t);
  const float inv_sqrt_bc2 = rsqrtf(bc2);
  const float d = ema_decay_at(ea, t), omd = 1.f - d;
  float* __restrict__ ema = ea.ema;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 pv = ((f32x4*)p)[i], gv = ((f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
    f32x4 ev;
    if constexpr (EMA) ev = ((f32x4*)ema)[i];             // with the other four streams, ahead of the table lookup
    const long a = tab.elem_base + (i << 2);
    long s = 0;
    vacnic_adamw_seg sg = {1.f, wd, 0, 0};
    bool whole = true;
    if constexpr (GROUPED) {
      s = seg_of(tab, a);
      sg = tab.seg[s];
      whole = a + 4 <= seg_end(tab, s);
    }
    if (whole) {                                          // the whole vector lies in one segment (all but a few vectors per boundary)
      if (!sg.frozen) {
        const float lr = GROUPED ? lr0 * sg.lr_scale : lr0;
        const float step_size = lr / bc1, decay = fmaf(-lr, sg.weight_decay, 1.f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float gr = gv[e] * gscale;
          const float me = adam_m(b1, mv[e], gr), ve = adam_v(b2, vv[e], gr);
          pv[e] = adam_p(pv[e], decay, step_size, me, ve, inv_sqrt_bc2, eps); mv[e] = me; vv[e] = ve;
          if constexpr (EMA) ev[e] = fmaf(d, ev[e], omd * pv[e]);
        }
        ((f32x4*)p)[i] = pv; ((f32x4*)m)[i] = mv; ((f32x4*)v)[i] = vv;
        if constexpr (EMA) ((f32x4*)ema)[i] = ev;
        if (pb) ((u32x2*)pb)[i] = (u32x2){pack2bf(pv[0], pv[1]), pack2bf(pv[2], pv[3])};
      }
    } else if constexpr (GROUPED) {                       // a boundary inside the vector: element by element, scalar stores
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
        if constexpr (EMA) ema[j] = fmaf(d, ev[e], omd * pe);
        if (pb) pb[j] = f2bf(pe);
      }
    }
    if (zero_grad) ((f32x4*)g)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};       // frozen elements too: backward still accumulates into them
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

// ---- gradient norm, pass 1, for clip_grad_norm_ and the non-finite gradient guard (include/vacnic_hip.h) --------------------
// Partial sums of (g * gscale)^2 over a fixed grid, in a fixed per-thread order, through a fixed-shape tree: the norm is
// bit-reproducible run to run (no float atomics) and the partial sums are the same bit for bit whichever entry point asks.
// GROUPED leaves out the frozen segments; GUARD also keeps, per block, the smallest absolute element index whose scaled gradient
// has a non-finite square.
constexpr int kNormBlocks = 1024;
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
template <bool GROUPED, bool GUARD>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long n4, float gscale,
                                                         float* __restrict__ partials, int64_t* __restrict__ first_idx,
                                                         GroupTable tab, const int64_t* __restrict__ hold) {
  if (hold && *hold == kHold) return;           // a held micro-batch: the arena is not read (uniform: the whole grid leaves)
  float acc = 0.f;
  long first = INT64_MAX;
  auto add = [&](float ge, long a) {                      // a rises within a thread: its first hit is its smallest
    const float x = ge * gscale;
    acc = fmaf(x, x, acc);
    if constexpr (GUARD) { if (nonfinite(x * x) && a < first) first = a; }
  };
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 gv = ((const f32x4*)g)[i];
    const long a = tab.elem_base + (i << 2);
    long s = 0;
    int frozen = 0;
    bool whole = true;
    if constexpr (GROUPED) {
      s = seg_of(tab, a);
      frozen = tab.seg[s].frozen;
      whole = a + 4 <= seg_end(tab, s);
    }
    if (whole) {
      if (!frozen) {
#pragma unroll
        for (int e = 0; e < 4; ++e) add(gv[e], a + e);
      }
    } else if constexpr (GROUPED) {                       // a boundary inside the vector
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (a + e >= seg_end(tab, s)) { s = seg_of(tab, a + e); frozen = tab.seg[s].frozen; }
        if (!frozen) add(gv[e], a + e);
      }
    }
  }
  if constexpr (GUARD) {
    guard_block_reduce(acc, first);
    if (threadIdx.x == 0) { partials[blockIdx.x] = acc; first_idx[blockIdx.x] = first; }
  } else {
    __shared__ float red[4];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}
// Pass 2 (one workgroup): grad_clip_coef_kernel's sum and coefficient, the verdict, the counters, and on a skip the undo of
// lr_step's increment of hyper[1].  skip <=> the sum of squares is not finite: squares cannot cancel, so that holds exactly when
// some element's square is non-finite or the fp32 sum itself overflowed (then no element is to blame: index -1).
__global__ __launch_bounds__(256) void grad_guard_verdict_kernel(const float* __restrict__ partials,
                                                                 const int64_t* __restrict__ first_idx, int nparts, float max_norm,
                                                                 float* __restrict__ out, int64_t* __restrict__ state,
                                                                 float* __restrict__ hyper, const int64_t* __restrict__ hold) {
  if (hold && *hold == kHold) {                 // a held micro-batch: the verdict is "hold", nothing is counted, out and hyper stay
    if (threadIdx.x == 0) state[0] = kHold;
    return;
  }
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

// ---- host side of the AdamW and norm entry points ---------------------------------------------------------------------------
// the table fields, which every args struct that has them carries under the same names (all three pointers null: no table)
template <class A> GroupTable table_of(const A* a) {
  return {a->seg_start, a->seg, a->first_seg, (long)a->nseg, (long)a->nblocks, (long)a->elem_base};
}
inline bool has_table(const GroupTable& t) { return t.seg_start || t.seg || t.first_seg; }
// ordering and coverage of the table are the host builder's to check (it lives in device memory: reading it here would sync)
int check_group_table(const GroupTable& t, int64_t n, const char* what) {
  VCHECK(t.seg_start && t.seg && t.first_seg, VACNIC_BAD_SHAPE, "%s: null group table", what);
  VCHECK(t.nseg >= 1 && t.nblocks >= 1 && t.elem_base >= 0, VACNIC_BAD_SHAPE,
         "%s: nseg=%ld and nblocks=%ld must be >= 1, elem_base=%ld >= 0", what, t.nseg, t.nblocks, t.elem_base);
  VCHECK(t.elem_base + n <= t.nblocks * 1024, VACNIC_BAD_SHAPE, "%s: elements [%ld, %ld) lie outside the table's %ld blocks of 1024",
         what, t.elem_base, (long)(t.elem_base + n), t.nblocks);
  return VACNIC_OK;
}

// What vacnic_adamw, vacnic_adamw_groups and vacnic_adamw_ema ask for, in one shape.  what: the name their messages carry;
// grouped: tab must be a whole table; with_ema: ema.ema must be set.
struct AdamwCall {
  const char* what;
  float *p, *g, *m, *v; void* p_bf16; const float* hyper; int64_t n;
  float beta1, beta2, eps, weight_decay, grad_scale; int32_t zero_grad;
  const float* clip_coef; const int64_t* skip;
  GroupTable tab; bool grouped;
  EmaArgs ema; bool with_ema;
};
int adamw_launch(const AdamwCall& c, void* stream) {
  VCHECK(c.p && c.g && c.m && c.v && c.hyper, VACNIC_BAD_SHAPE, "%s: null operand", c.what);
  VCHECK(!c.with_ema || c.ema.ema, VACNIC_BAD_SHAPE, "%s: null ema", c.what);
  VCHECK(c.n >= 0 && (c.n & 3) == 0, VACNIC_BAD_SHAPE, "%s: n=%ld must be a multiple of 4 (pad the arena)", c.what, (long)c.n);
  VCHECK(!c.with_ema || (c.ema.decay > 0.f && c.ema.decay < 1.f), VACNIC_BAD_SHAPE, "%s: ema_decay=%g must lie in (0, 1)", c.what,
         (double)c.ema.decay);
  VCHECK(aligned16(c.p) && aligned16(c.g) && aligned16(c.m) && aligned16(c.v) && (!c.with_ema || aligned16(c.ema.ema)) &&
             (!c.p_bf16 || (((uintptr_t)c.p_bf16) & 7) == 0),
         VACNIC_MISALIGNED, "%s: arenas must be 16-byte aligned", c.what);
  if (c.grouped) {
    if (const int err = check_group_table(c.tab, c.n, c.what)) return err;
  } else {
    VCHECK(c.tab.elem_base >= 0, VACNIC_BAD_SHAPE, "%s: elem_base=%ld must be >= 0", c.what, c.tab.elem_base);
  }
  if (c.n == 0) return VACNIC_OK;
  const long n4 = c.n >> 2;
  unsigned blocks = 65536;                     // wide launch (see the kernel comment); small arenas: one element per thread
  const long need = (n4 + 255) / 256;
  if (need < blocks) blocks = (unsigned)need;
  const auto kernel = c.grouped ? (c.with_ema ? adamw_kernel<true, true> : adamw_kernel<true, false>)
                                : (c.with_ema ? adamw_kernel<false, true> : adamw_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, c.p, c.g, c.m, c.v, (bf16_t*)c.p_bf16, c.hyper, n4,
                     c.beta1, c.beta2, c.eps, c.weight_decay, c.grad_scale, c.zero_grad, c.clip_coef, c.tab, c.skip, c.ema);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

// pass 1 of the norm: a table picks GROUPED (without one only tab.elem_base counts), first_idx picks GUARD
void launch_grad_sumsq(const float* g, int64_t n, float gscale, float* partials, int64_t* first_idx, const GroupTable& tab,
                       const int64_t* hold, void* stream) {
  const auto kernel = has_table(tab) ? (first_idx ? grad_sumsq_kernel<true, true> : grad_sumsq_kernel<true, false>)
                                     : (first_idx ? grad_sumsq_kernel<false, true> : grad_sumsq_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(kNormBlocks), dim3(256), 0, (hipStream_t)stream, g, (long)(n >> 2), gscale, partials, first_idx, tab,
                     hold);
}

}  // namespace

extern "C" int vacnic_lr_step(float* hyper, float base_lr, float warmup_steps, float total_steps, uint64_t* rng_counter, void* stream) {
  VPLAN_REC(vacnic_lr_step, hyper, base_lr, warmup_steps, total_steps, rng_counter, stream);
  VCHECK(hyper, VACNIC_BAD_SHAPE, "lr_step: null hyper");
  hipLaunchKernelGGL(lr_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hyper, base_lr, warmup_steps, total_steps, (unsigned long long*)rng_counter);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int vacnic_lr_step_accum(float* hyper, float base_lr, float warmup_steps, float total_steps, uint64_t* rng_counter,
                                    int64_t* accum, int32_t k, void* stream) {
  VPLAN_REC(vacnic_lr_step_accum, hyper, base_lr, warmup_steps, total_steps, rng_counter, accum, k, stream);
  VCHECK(hyper && accum, VACNIC_BAD_SHAPE, "lr_step_accum: null operand");
  VCHECK(k >= 1, VACNIC_BAD_SHAPE, "lr_step_accum: k=%d micro-batches per optimizer step must be >= 1", (int)k);
  VCHECK(((uintptr_t)accum & 7) == 0, VACNIC_MISALIGNED, "lr_step_accum: accum must be 8-byte aligned");
  hipLaunchKernelGGL(lr_step_accum_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hyper, base_lr, warmup_steps, total_steps,
                     (unsigned long long*)rng_counter, accum, (int)k);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int vacnic_adamw(const vacnic_adamw_args* a, void* stream) {
  VPLAN_REC_STRUCT(vacnic_adamw, a, stream);
  VCHECK(a, VACNIC_BAD_SHAPE, "adamw: null operand");
  return adamw_launch({"adamw", a->p, a->g, a->m, a->v, a->p_bf16, a->hyper, a->n, a->beta1, a->beta2, a->eps, a->weight_decay,
                       a->grad_scale, a->zero_grad, a->clip_coef, a->skip, GroupTable{}, false, EmaArgs{}, false}, stream);
}

extern "C" int vacnic_grad_clip_coef(const float* g, int64_t n, float grad_scale, float max_norm, float* partials,
                                     float* out, void* stream) {
  VPLAN_REC(vacnic_grad_clip_coef, g, n, grad_scale, max_norm, partials, out, stream);
  VCHECK(g && partials && out, VACNIC_BAD_SHAPE, "grad_clip_coef: null operand");
  VCHECK((n & 3) == 0 && aligned16(g), VACNIC_BAD_SHAPE, "grad_clip_coef: arena must be 16-byte aligned, n=%ld a multiple of 4", (long)n);
  VCHECK(max_norm > 0.f, VACNIC_BAD_SHAPE, "grad_clip_coef: max_norm must be > 0");
  launch_grad_sumsq(g, n, grad_scale, partials, nullptr, GroupTable{}, nullptr, stream);
  VLAUNCH_CHECK();
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, kNormBlocks, max_norm, out,
                     (const int64_t*)nullptr);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int vacnic_adamw_groups(const vacnic_adamw_groups_args* a, void* stream) {
  VPLAN_REC_STRUCT(vacnic_adamw_groups, a, stream);
  VCHECK(a, VACNIC_BAD_SHAPE, "adamw_groups: null operand");
  return adamw_launch({"adamw_groups", a->p, a->g, a->m, a->v, a->p_bf16, a->hyper, a->n, a->beta1, a->beta2, a->eps, 0.f,
                       a->grad_scale, a->zero_grad, a->clip_coef, a->skip, table_of(a), true, EmaArgs{}, false}, stream);
}

extern "C" int vacnic_adamw_ema(const vacnic_adamw_ema_args* a, void* stream) {
  VPLAN_REC_STRUCT(vacnic_adamw_ema, a, stream);
  VCHECK(a, VACNIC_BAD_SHAPE, "adamw_ema: null operand");
  const GroupTable tab = table_of(a);
  return adamw_launch({"adamw_ema", a->p, a->g, a->m, a->v, a->p_bf16, a->hyper, a->n, a->beta1, a->beta2, a->eps, a->weight_decay,
                       a->grad_scale, a->zero_grad, a->clip_coef, a->skip, tab, has_table(tab),
                       EmaArgs{a->ema, a->ema_decay, a->ema_warmup}, true}, stream);
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
  VCHECK(a->elem_base >= 0, VACNIC_BAD_SHAPE, "grad_clip_coef_groups: elem_base=%ld must be >= 0", (long)a->elem_base);
  VCHECK(((uintptr_t)a->hold & 7) == 0, VACNIC_MISALIGNED, "grad_clip_coef_groups: hold must be 8-byte aligned");
  const GroupTable tab = table_of(a);
  if (has_table(tab)) {                          // null table pointers: ungrouped, as vacnic_grad_guard reads them
    if (const int err = check_group_table(tab, a->n, "grad_clip_coef_groups")) return err;
  }
  launch_grad_sumsq(a->g, a->n, a->grad_scale, a->partials, nullptr, tab, a->hold, stream);
  VLAUNCH_CHECK();
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a->partials, kNormBlocks, a->max_norm, a->out,
                     a->hold);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}

extern "C" int vacnic_grad_guard(const vacnic_grad_guard_args* a, void* stream) {
  VPLAN_REC_STRUCT(vacnic_grad_guard, a, stream);
  VCHECK(a && a->g && a->partials && a->first_idx && a->out && a->state && a->hyper, VACNIC_BAD_SHAPE, "grad_guard: null operand");
  VCHECK(a->n >= 0 && (a->n & 3) == 0 && aligned16(a->g), VACNIC_BAD_SHAPE,
         "grad_guard: arena must be 16-byte aligned, n=%ld a multiple of 4", (long)a->n);
  VCHECK(a->elem_base >= 0, VACNIC_BAD_SHAPE, "grad_guard: elem_base=%ld must be >= 0", (long)a->elem_base);
  VCHECK(((uintptr_t)a->first_idx & 7) == 0 && ((uintptr_t)a->state & 7) == 0 && ((uintptr_t)a->hold & 7) == 0, VACNIC_MISALIGNED,
         "grad_guard: first_idx, state and hold must be 8-byte aligned");
  const GroupTable tab = table_of(a);
  if (has_table(tab)) {
    if (const int err = check_group_table(tab, a->n, "grad_guard")) return err;
  }
  launch_grad_sumsq(a->g, a->n, a->grad_scale, a->partials, a->first_idx, tab, a->hold, stream);
  VLAUNCH_CHECK();
  hipLaunchKernelGGL(grad_guard_verdict_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a->partials, a->first_idx, kNormBlocks,
                     a->max_norm, a->out, a->state, a->hyper, a->hold);
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
