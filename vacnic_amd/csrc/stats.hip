// Per-parameter gradient and weight statistics over the flat arenas (vacnic_param_stats, include/vacnic_hip.h): what
// wandb.watch(model) (TRAIN:456) gives the reference's users, as a segmented, bit-reproducible reduction that is gated on the
// device, so a launch plan or a hipGraph can carry it.  HBM-bound when it fires (8 B per element: g and p); when it does not,
// two launches whose workgroups read the gate and leave.
#include "common.h"

namespace {

constexpr int kUnit = 4096;            // a unit never holds more elements: the host's cut, and the clamp of a malformed one
constexpr int kPass1Blocks = 1024;     // upper bound of the pass-1 grid, the norm pass's (optim.hip): 4 four-wave workgroups per CU, all
                                       // resident at this kernel's 5 waves per SIMD, and few enough that a gated-off launch is cheap

// as the guard defines it (optim.hip): the fp32 square of the scaled gradient is NaN or Inf
__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// The gate, evaluated by both passes from the same two device values (nothing between the passes writes them).
struct Gate { long t; int on_skip; bool fire; };
__device__ __forceinline__ Gate read_gate(const float* __restrict__ hyper, int every, const int64_t* __restrict__ skip) {
  Gate g;
  g.t = hyper ? (long)hyper[1] : -1;
  const int64_t word = skip ? *skip : 0;        // the step word (optim.hip): 0 apply, 1 dropped by the guard, 2 hold
  g.on_skip = word != 0 ? 1 : 0;
  // a held micro-batch of an accumulation group never fires: the gradient is a partial sum, and hyper[1] has not moved
  g.fire = word != 2 && (!hyper || g.on_skip || (g.t % every) == 0);
  return g;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long wave_sum_i64(long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (long)__shfl_xor((long long)v, o, 64);
  return v;
}

// one thread's running statistics
struct Acc {
  float gsq = 0.f, gmax = 0.f, psq = 0.f, pmax = 0.f;
  int bad = 0, zeros = 0;
  __device__ __forceinline__ void grad(float ge, float gscale) {
    const float x = ge * gscale;
    const bool nf = nonfinite(x * x);
    const float xs = nf ? 0.f : x;                // a non-finite element adds 0 to the sum, 0 to the maximum and 1 to the count
    gsq = fmaf(xs, xs, gsq);
    gmax = fmaxf(gmax, fabsf(xs));
    bad += nf ? 1 : 0;
    zeros += ge == 0.f ? 1 : 0;
  }
  __device__ __forceinline__ void weight(float pe) {
    psq = fmaf(pe, pe, psq);
    pmax = fmaxf(pmax, fabsf(pe));
  }
};

// Pass 1: one WAVE per unit, the waves of a fixed grid striding over the units.  A lane takes the unit's 16-byte vectors
// lane, lane + 64, ... in rising order (at most 16 of them: 64 terms per sum), the up to three elements before the first aligned
// vector and after the last one with scalar loads, and the wave folds its 64 lanes through the xor butterfly: a unit's partial
// depends on the unit alone, not on the grid or on which wave took it.  Every unit's partial is written, an empty one's too.
template <bool HAS_P>
__global__ __launch_bounds__(256) void param_stats_units_kernel(const float* __restrict__ g, const float* __restrict__ p, long n,
                                                                float gscale, const int64_t* __restrict__ unit_off,
                                                                const int32_t* __restrict__ unit_len, long nunit,
                                                                const float* __restrict__ hyper, int every,
                                                                const int64_t* __restrict__ skip, f32x4* __restrict__ part_f,
                                                                int2* __restrict__ part_i) {
  if (!read_gate(hyper, every, skip).fire) return;
  const int lane = threadIdx.x & 63;
  const long nwaves = (long)gridDim.x * 4;
  for (long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6); u < nunit; u += nwaves) {
    // clamped into [0, n) and to kUnit elements: a malformed table gives wrong values, never an access outside the arenas
    long off = unit_off[u], len = unit_len[u];
    off = off < 0 ? 0 : (off > n ? n : off);
    len = len < 0 ? 0 : (len > kUnit ? kUnit : len);
    const long end = off + len > n ? n : off + len;
    long a0 = (off + 3) & ~3L;                                  // first aligned vector
    a0 = a0 > end ? end : a0;
    long a1 = end & ~3L;                                        // end of the last whole vector
    a1 = a1 < a0 ? a0 : a1;
    Acc acc;
    if (off + lane < a0) {                                      // head: lanes 0..2
      acc.grad(g[off + lane], gscale);
      if constexpr (HAS_P) acc.weight(p[off + lane]);
    }
#pragma unroll 4
    for (long i = (a0 >> 2) + lane; i < (a1 >> 2); i += 64) {
      const f32x4 gv = ((const f32x4*)g)[i];
      f32x4 pv;
      if constexpr (HAS_P) pv = ((const f32x4*)p)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc.grad(gv[e], gscale);
        if constexpr (HAS_P) acc.weight(pv[e]);
      }
    }
    if (a1 + lane < end) {                                      // tail: lanes 0..2
      acc.grad(g[a1 + lane], gscale);
      if constexpr (HAS_P) acc.weight(p[a1 + lane]);
    }
    const float gsq = wave_sum(acc.gsq), gmax = wave_max(acc.gmax);
    const float psq = HAS_P ? wave_sum(acc.psq) : 0.f, pmax = HAS_P ? wave_max(acc.pmax) : 0.f;
    const int bad = wave_sum_i32(acc.bad), zeros = wave_sum_i32(acc.zeros);
    if (lane == 0) {
      part_f[u] = (f32x4){gsq, gmax, psq, pmax};
      part_i[u] = make_int2(bad, zeros);
    }
  }
}

// Pass 2: one workgroup per slot folds the slot's contiguous run of unit partials: thread t takes partials t, t + 256, ... of the
// run in rising order, then the wave butterfly and the fixed (0 + 1) + (2 + 3) over the four waves.  Workgroup 0 writes the stamp.
__global__ __launch_bounds__(256) void param_stats_slots_kernel(const f32x4* __restrict__ part_f, const int2* __restrict__ part_i,
                                                                const int64_t* __restrict__ slot_unit, long nunit,
                                                                const float* __restrict__ hyper, int every,
                                                                const int64_t* __restrict__ skip, float* __restrict__ out_f,
                                                                int64_t* __restrict__ out_i, int64_t* __restrict__ stamp) {
  const Gate gate = read_gate(hyper, every, skip);
  if (!gate.fire) return;
  const long s = blockIdx.x;
  long u0 = slot_unit[s], u1 = slot_unit[s + 1];
  u0 = u0 < 0 ? 0 : (u0 > nunit ? nunit : u0);
  u1 = u1 < u0 ? u0 : (u1 > nunit ? nunit : u1);
  float gsq = 0.f, gmax = 0.f, psq = 0.f, pmax = 0.f;
  long bad = 0, zeros = 0;
  for (long u = u0 + threadIdx.x; u < u1; u += 256) {
    const f32x4 f = part_f[u];
    const int2 c = part_i[u];
    gsq += f[0]; gmax = fmaxf(gmax, f[1]); psq += f[2]; pmax = fmaxf(pmax, f[3]);
    bad += c.x; zeros += c.y;
  }
  __shared__ float redf[4][4];
  __shared__ long redi[4][2];
  gsq = wave_sum(gsq); gmax = wave_max(gmax); psq = wave_sum(psq); pmax = wave_max(pmax);
  bad = wave_sum_i64(bad); zeros = wave_sum_i64(zeros);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    redf[w][0] = gsq; redf[w][1] = gmax; redf[w][2] = psq; redf[w][3] = pmax;
    redi[w][0] = bad; redi[w][1] = zeros;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out_f[4 * s + 0] = (redf[0][0] + redf[1][0]) + (redf[2][0] + redf[3][0]);
    out_f[4 * s + 1] = fmaxf(fmaxf(redf[0][1], redf[1][1]), fmaxf(redf[2][1], redf[3][1]));
    out_f[4 * s + 2] = (redf[0][2] + redf[1][2]) + (redf[2][2] + redf[3][2]);
    out_f[4 * s + 3] = fmaxf(fmaxf(redf[0][3], redf[1][3]), fmaxf(redf[2][3], redf[3][3]));
    out_i[2 * s + 0] = (redi[0][0] + redi[1][0]) + (redi[2][0] + redi[3][0]);
    out_i[2 * s + 1] = (redi[0][1] + redi[1][1]) + (redi[2][1] + redi[3][1]);
    if (s == 0) {
      stamp[0] += 1; stamp[1] = gate.t; stamp[2] = gate.on_skip; stamp[3] = 0;
    }
  }
}

}  // namespace

extern "C" int64_t vacnic_param_stats_workspace_bytes(int64_t nunit, int64_t nslot) {
  (void)nslot;                         // pass 2 writes the results directly: the workspace holds the unit partials only
  return nunit < 0 ? 0 : nunit * (int64_t)(sizeof(f32x4) + sizeof(int2));
}

extern "C" int vacnic_param_stats(const vacnic_param_stats_args* a, void* stream) {
  VPLAN_REC_STRUCT(vacnic_param_stats, a, stream);
  VCHECK(a && a->g && a->unit_off && a->unit_len && a->slot_unit && a->workspace && a->out_f && a->out_i && a->stamp,
         VACNIC_BAD_SHAPE, "param_stats: null operand");
  VCHECK(a->n >= 0, VACNIC_BAD_SHAPE, "param_stats: n=%ld must be >= 0", (long)a->n);
  VCHECK(a->nslot >= 1 && a->nunit >= 1, VACNIC_BAD_SHAPE, "param_stats: nslot=%ld and nunit=%ld must be >= 1", (long)a->nslot,
         (long)a->nunit);
  VCHECK(a->every >= 1, VACNIC_BAD_SHAPE, "param_stats: every=%d must be >= 1", (int)a->every);
  VCHECK(a->workspace_bytes >= vacnic_param_stats_workspace_bytes(a->nunit, a->nslot), VACNIC_BAD_SHAPE,
         "param_stats: workspace of %ld bytes, %ld needed (vacnic_param_stats_workspace_bytes)", (long)a->workspace_bytes,
         (long)vacnic_param_stats_workspace_bytes(a->nunit, a->nslot));
  VCHECK(aligned16(a->g) && (!a->p || aligned16(a->p)) && aligned16(a->workspace), VACNIC_MISALIGNED,
         "param_stats: g, p and the workspace must be 16-byte aligned");
  VCHECK(((uintptr_t)a->out_i & 7) == 0 && ((uintptr_t)a->stamp & 7) == 0 && ((uintptr_t)a->unit_off & 7) == 0 &&
             ((uintptr_t)a->slot_unit & 7) == 0 && ((uintptr_t)a->skip & 7) == 0,
         VACNIC_MISALIGNED, "param_stats: the int64 operands must be 8-byte aligned");
  f32x4* part_f = (f32x4*)a->workspace;
  int2* part_i = (int2*)(part_f + a->nunit);
  const long need = (a->nunit + 3) / 4;
  const unsigned blocks = (unsigned)(need < kPass1Blocks ? need : kPass1Blocks);
  const auto units = a->p ? param_stats_units_kernel<true> : param_stats_units_kernel<false>;
  hipLaunchKernelGGL(units, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a->g, a->p, (long)a->n, a->grad_scale, a->unit_off,
                     a->unit_len, (long)a->nunit, a->hyper, (int)a->every, a->skip, part_f, part_i);
  VLAUNCH_CHECK();
  hipLaunchKernelGGL(param_stats_slots_kernel, dim3((unsigned)a->nslot), dim3(256), 0, (hipStream_t)stream, part_f, part_i,
                     a->slot_unit, (long)a->nunit, a->hyper, (int)a->every, a->skip, a->out_f, a->out_i, a->stamp);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}
