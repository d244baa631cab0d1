// Sampling decode (transformers 4.18 GenerationMixin.sample): logits processors -> temperature -> top-k -> top-p -> one draw,
// plus the bookkeeping of the position, in ONE launch per position, one 1024-thread workgroup per row.  The exact semantics
// (order of operations, tie rules, Philox key / counter layout, the u formula, the fixed-point masses) are specified in
// include/vacnic_hip.h at vacnic_sample_step; this file follows that comment step by step.
//
// Layout: the row (V <= 65536 fp32 logits) is read ONCE and lives in registers as order-preserving 32-bit keys, <= 64 per lane:
// wave w owns the contiguous ids [w * nper * 64, (w + 1) * nper * 64), lane l its elements i * 64 + l (256-byte coalesced loads),
// nper = ceil(V / 1024).  Both selections are MSB-first radix selects over the keys (4 passes of 8 bits, integer compares only):
// top-k by element COUNT, top-p by probability MASS.  Masses are integers, q = rint(exp(z' - max z') * 2^31), so every sum in
// this kernel (histograms by LDS integer atomics, totals, the cumulative sum of the draw) is exact and independent of the
// order it is formed in: two launches on the same inputs give the same bits, and there is no floating-point atomic anywhere.
// Histograms are kept in 8 copies (lane & 7) with a row stride of 257 words: the top digits of a row of logits fall into a
// handful of bins, and same-address LDS atomics of one wave serialise.
#include "common.h"
#include <float.h>

namespace {

constexpr int ST = 1024, SWAVES = 16, SNPT = 64, SCOPY = 8, SBINS = 256, SSTRIDE = 257;
constexpr uint32_t KEY_NINF = 0x007fffffu;        // key of -inf; key 0 = "no element" (below every real key)
constexpr uint32_t SAMPLE_TAG = 0x53414D50u;      // "SAMP": Philox counter word 2 of this kernel
typedef unsigned long long u64;

// float -> uint32, monotone: a < b  <=>  key(a) < key(b) (no NaN, -0 canonicalised to +0 by the caller)
__device__ __forceinline__ uint32_t f2key(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <class T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct SampleP {
  const float* logits; const uint32_t* params; int32_t* seq; int32_t* done; int64_t* next_ids; float* logp;
  int32_t* kept; float* thr; float* mass; float* u;
  const int32_t* bad_words; const int32_t* bad_len;
  long ldl;
  int V, Lmax, cur_len, eos, pad, ngram, suppress_eos, forced, n_bad;
};

__global__ __launch_bounds__(ST) void sample_step_kernel(SampleP p) {
  __shared__ uint32_t banbits[2048];                      // one bit per token id (V <= 65536)
  __shared__ uint32_t histbits[2048];                     // tokens of the row's history (repetition penalty)
  __shared__ uint32_t hcnt[SCOPY * SSTRIDE];
  __shared__ u64 hmass[SCOPY * SSTRIDE];
  __shared__ uint32_t bcnt[SBINS];
  __shared__ u64 bmass[SBINS];
  __shared__ uint32_t wred[SWAVES], wkept[SWAVES];
  __shared__ u64 wtot[SWAVES];
  __shared__ uint32_t sel_bin;
  __shared__ u64 sel_before, sel_limit, sel_total;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), V = p.V;
  const long r = blockIdx.x;

  // ---- runtime parameters (device memory: a captured launch serves every setting)
  float T = __uint_as_float(p.params[0]);
  if (!(T > 0.f)) T = 1.f;
  const int top_k = (int)p.params[1];
  const float top_p = __uint_as_float(p.params[2]);
  float pen = __uint_as_float(p.params[3]);               // repetition penalty; the 0 of a block written without one reads as 1 = off
  if (!(pen > 0.f)) pen = 1.f;
  const bool penal = pen != 1.f;
  const u64 seed = (u64)p.params[4] | ((u64)p.params[5] << 32), call = (u64)p.params[6] | ((u64)p.params[7] << 32);
  const u64 pkey = seed + 0x9E3779B97F4A7C15ull * call;
  uint32_t rnd[4];
  philox4x32((uint32_t)r, (uint32_t)p.cur_len, SAMPLE_TAG, 0u, (uint32_t)pkey, (uint32_t)(pkey >> 32), rnd);
  const uint32_t m24 = rnd[0] >> 8;
  const size_t so = (size_t)r * p.Lmax + p.cur_len;
  if (tid == 0 && p.u) p.u[r] = (float)(((double)m24 + 0.5) * (1.0 / 16777216.0));

  auto finish = [&](int token, float lp, int nkept, float thr, float mass, bool ends) {      // one thread
    p.next_ids[r] = token;
    p.seq[so] = token;
    if (p.logp) p.logp[so] = lp;
    if (ends) p.done[r] = 1;
    if (p.kept) p.kept[r] = nkept;
    if (p.thr) p.thr[r] = thr;
    if (p.mass) p.mass[r] = mass;
  };
  // ---- 1. processors that need no logits: a finished row pads, a forced token is certain
  if (p.done[r] != 0) {
    if (tid == 0) finish(p.pad, 0.f, 0, 0.f, 0.f, false);
    return;
  }
  if (p.forced >= 0) {
    if (tid == 0) finish(p.forced, 0.f, 1, 0.f, 1.f, p.forced == p.eos);
    return;
  }
  // NoRepeatNGram: the tokens that followed an earlier occurrence of the last n - 1 tokens of this row's history
  const int n = p.ngram;
  const bool grams = n > 0 && p.cur_len + 1 >= n;
  const bool bans = grams || p.n_bad > 0;
  if (bans || penal) {
    for (int w = tid; w < 2048; w += ST) { banbits[w] = 0u; histbits[w] = 0u; }
    __syncthreads();
    const int32_t* h = p.seq + (size_t)r * p.Lmax;
    const int len = p.cur_len;
    if (grams) {
      for (int i = tid; i <= len - n; i += ST) {
        bool match = true;
        for (int k = 0; k < n - 1; ++k) match = match && h[i + k] == h[len - (n - 1) + k];
        const int t = h[i + n - 1];
        if (match && t >= 0 && t < V) atomicOr(&banbits[t >> 5], 1u << (t & 31));
      }
    }
    // NoBadWords: word w of m tokens bans w[m - 1] if the last m - 1 history tokens are w[0 .. m - 2] (m - 1 <= cur_len)
    for (int w = tid; w < p.n_bad; w += ST) {
      const int m = p.bad_len[w];
      if (m < 1 || m > VACNIC_BAD_WORD_LEN || m - 1 > len) continue;
      const int32_t* bw = p.bad_words + (size_t)w * VACNIC_BAD_WORD_LEN;
      bool match = true;
      for (int k = 0; k < m - 1; ++k) match = match && bw[k] == h[len - (m - 1) + k];
      const int t = bw[m - 1];
      if (match && t >= 0 && t < V) atomicOr(&banbits[t >> 5], 1u << (t & 31));
    }
    if (penal) {
      for (int i = tid; i < len; i += ST) {
        const int t = h[i];
        if (t >= 0 && t < V) atomicOr(&histbits[t >> 5], 1u << (t & 31));
      }
    }
    __syncthreads();
  }
  // ---- 1 + 2. the row -> keys of z' = z / T (IEEE division), banned / suppressed tokens -inf
  const float* row = p.logits + (size_t)r * p.ldl;
  const int nper = (V + ST - 1) / ST;
  const int base = wave * nper * 64;
  const int wend = base + nper * 64 < V ? base + nper * 64 : V;             // this wave's ids are [base, wend)
  uint32_t key[SNPT];
  uint32_t kmax = 0u;
  // f(i) over this lane's elements, fully unrolled (key[] stays in registers) in 8 groups of 8 behind ONE uniform test each; an
  // element beyond the wave's range has key 0.  The scheduling barrier keeps the iterations apart: interleaved, their temporaries spill.
  auto for_keys = [&](auto&& f) {
#pragma unroll
    for (int g = 0; g < SNPT / 8; ++g) {
      if (g * 8 < nper) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          f(g * 8 + e);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  };
#pragma unroll
  for (int i = 0; i < SNPT; ++i) key[i] = 0u;
#pragma unroll
  for (int g = 0; g < SNPT / 8; ++g) {                                      // all loads of the row in flight before the first use
    if (g * 8 < nper) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = base + (g * 8 + e) * 64 + lane;
        if (j < wend) key[g * 8 + e] = __float_as_uint(row[j]);
      }
    }
  }
  int Vt = wend;
  asm volatile("" : "+s"(Vt));                                              // (keeps 64 load predicates from staying live as masks)
  if (penal) {
    // RepetitionPenalty on the raw logits, once per distinct history token — a sweep of its own behind one uniform test, so that
    // the sweep below is the one of a call without a penalty
    for_keys([&](int i) {
      const int j = base + i * 64 + lane;
      if (j < Vt && ((histbits[j >> 5] >> (j & 31)) & 1u)) {
        float z = __uint_as_float(key[i]);
        z = z != z ? -INFINITY : fminf(z, FLT_MAX);
        key[i] = __float_as_uint(z < 0.f ? __fmul_rn(z, pen) : __fdiv_rn(z, pen));
      }
    });
  }
  for_keys([&](int i) {
    {
      const int j = base + i * 64 + lane;
      if (j < Vt) {
        float zp = __fdiv_rn(__uint_as_float(key[i]), T);
        zp = zp != zp ? -INFINITY : fminf(zp, FLT_MAX);
        if (zp == 0.f) zp = 0.f;                                            // -0 -> +0: one key per value
        if ((p.suppress_eos && j == p.eos) || (bans && ((banbits[j >> 5] >> (j & 31)) & 1u))) zp = -INFINITY;
        key[i] = f2key(zp);
        kmax = kmax > key[i] ? kmax : key[i];
      }
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)kmax, o, 64);
    kmax = kmax > t ? kmax : t;
  }
  if (lane == 0) wred[wave] = kmax;
  __syncthreads();
  kmax = wred[0];
#pragma unroll
  for (int w = 1; w < SWAVES; ++w) kmax = kmax > wred[w] ? kmax : wred[w];
  if (kmax <= KEY_NINF) {                                                   // no finite logit: the row ends
    if (tid == 0) finish(p.eos, 0.f, 0, -INFINITY, 0.f, true);
    return;
  }
  const float zmax = key2f(kmax);
  // fixed-point unnormalised probability, <= 2^31.  Every sweep over the keys passes its own opaque copy of zmax: the masses are
  // recomputed per sweep on purpose (64 more live registers per lane would spill), which the optimiser would otherwise undo by
  // hoisting them out of the pass loop or sharing them between sweeps.
  auto opaque = [](float v) -> float { asm volatile("" : "+v"(v)); return v; };
  auto qmass = [&](uint32_t k, float zm) -> uint32_t {
    return k <= KEY_NINF ? 0u : __float2uint_rn(expf(key2f(k) - zm) * 2147483648.f);
  };

  // MSB-first radix select over the elements with key >= lo.  by_mass = false: the `want`-th largest key (counting duplicates).
  // by_mass = true: the smallest present key whose mass of STRICTLY larger keys is <= top_p * (mass of all of them).
  auto radix_select = [&](bool by_mass, uint32_t lo, uint32_t want) -> uint32_t {
    uint32_t prefix = 0u, pmask = 0u;
    u64 carry = 0;                                                          // mass above the prefix's bin (by_mass)
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      for (int w = tid; w < SCOPY * SSTRIDE; w += ST) { hcnt[w] = 0u; hmass[w] = 0; }
      __syncthreads();
      const int copy = (lane & (SCOPY - 1)) * SSTRIDE;
      const float zm = opaque(zmax);
      const uint32_t lo_ = __float_as_uint(opaque(__uint_as_float(lo)));
      for_keys([&](int i) {
        const uint32_t k = key[i];
        if (k != 0u && k >= lo_ && (k & pmask) == prefix) {
          const int bin = (k >> shift) & 255;
          atomicAdd(&hcnt[copy + bin], 1u);
          if (by_mass) atomicAdd(&hmass[copy + bin], (u64)qmass(k, zm));
        }
      });
      __syncthreads();
      if (tid < SBINS) {
        uint32_t c = 0u; u64 m = 0;
#pragma unroll
        for (int cp = 0; cp < SCOPY; ++cp) { c += hcnt[cp * SSTRIDE + tid]; m += hmass[cp * SSTRIDE + tid]; }
        bcnt[tid] = c; bmass[tid] = m;
      }
      __syncthreads();
      if (wave == 0) {
        // lane l looks at bins 255 - 4 l .. 252 - 4 l: ascending lanes walk the keys downwards
        uint32_t c[4]; u64 m[4];
        uint32_t ct = 0u; u64 mt = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) { c[e] = bcnt[255 - 4 * lane - e]; m[e] = bmass[255 - 4 * lane - e]; ct += c[e]; mt += m[e]; }
        uint32_t cb = wave_incl_scan(ct, lane) - ct;                        // elements / mass in the bins above this lane's
        u64 mb = wave_incl_scan(mt, lane) - mt;
        if (!by_mass) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (cb < want && want <= cb + c[e]) { sel_bin = 255 - 4 * lane - e; sel_before = cb; }
            cb += c[e];
          }
        } else {
          u64 limit = sel_limit;
          if (pass == 0) {                                                  // floor(top_p * Z): E <= top_p * Z  <=>  E <= floor(..) for an integer E
            const u64 total = wave_sum_u64(mt);
            limit = (u64)((double)top_p * (double)total);
            if (lane == 0) { sel_total = total; sel_limit = limit; }
          }
          int cand = -1; u64 cand_before = 0;
          mb += carry;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (c[e] > 0u && mb <= limit) { cand = 255 - 4 * lane - e; cand_before = mb; }
            mb += m[e];
          }
          const u64 have = __ballot(cand >= 0);
          if (have != 0 && lane == 63 - __clzll((long long)have)) { sel_bin = cand; sel_before = cand_before; }
        }
      }
      __syncthreads();
      prefix |= sel_bin << shift;
      pmask |= 255u << shift;
      if (by_mass) carry = sel_before; else want -= (uint32_t)sel_before;
    }
    return prefix;
  };

  // ---- 3. top-k: keep z' >= the k-th largest z' (ties all kept)
  uint32_t lo = 0u;
  if (top_k >= 1 && top_k < V) lo = radix_select(false, 0u, (uint32_t)top_k);
  // ---- 4. top-p over what is left: keep v iff mass{z' > z'_v} <= top_p * mass{left}
  const bool nucleus = top_p > 0.f && top_p < 1.f;
  u64 zact = 0;
  if (nucleus) {
    lo = radix_select(true, lo, 0u);
    zact = sel_total;
  }
  if (lo < KEY_NINF) lo = KEY_NINF;                                         // thr = -inf: everything is "kept", only finite tokens count
  // ---- 5. the draw: first kept token in ascending id whose inclusive cumulative mass exceeds u * Z
  u64 msum = 0; uint32_t nk = 0u;
  const float zm1 = opaque(zmax);
  for_keys([&](int i) {
    const uint32_t k = key[i];
    if (k >= lo && k > KEY_NINF) { msum += qmass(k, zm1); ++nk; }
  });
  msum = wave_sum_u64(msum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nk += (uint32_t)__shfl_xor((int)nk, o, 64);
  if (lane == 0) { wtot[wave] = msum; wkept[wave] = nk; }
  __syncthreads();
  u64 Z = 0; uint32_t nkept = 0u;
#pragma unroll
  for (int w = 0; w < SWAVES; ++w) { Z += wtot[w]; nkept += wkept[w]; }
  // target = floor(u * Z) with u = (2 m24 + 1) / 2^25 exactly: cum > u * Z  <=>  cum > floor(u * Z) for an integer cum
  const u64 odd = 2ull * m24 + 1ull;
  const u64 target = odd * (Z >> 25) + ((odd * (Z & 0x1ffffffull)) >> 25);
  u64 run = 0; int wsel = SWAVES - 1;
  for (int w = 0; w < SWAVES; ++w) {
    if (target < run + wtot[w]) { wsel = w; break; }
    run += wtot[w];
  }
  if (wave != wsel) return;
  bool found = false;
  const float zm2 = opaque(zmax);
  for_keys([&](int i) {
    if (!found) {
      const uint32_t k = key[i];
      const u64 m = (k >= lo && k > KEY_NINF) ? (u64)qmass(k, zm2) : 0ull;
      const u64 s = wave_incl_scan(m, lane);
      const u64 hit = __ballot(run + s > target);
      if (hit != 0) {
        found = true;
        if (lane == __ffsll((long long)hit) - 1) {
          const int token = base + i * 64 + lane;
          const float lp = (key2f(k) - zmax) - (float)log((double)Z * (1.0 / 2147483648.0));
          finish(token, lp, (int)nkept, key2f(lo), nucleus ? (float)((double)Z / (double)zact) : 1.f, token == p.eos);
        }
      }
      run += __shfl(s, 63, 64);
    }
  });
}
}  // namespace

extern "C" int vacnic_sample_step(const vacnic_sample_step_args* a, void* stream) {
  VPLAN_REC_STRUCT(vacnic_sample_step, a, stream);
  VCHECK(a && a->logits && a->params && a->seq && a->done && a->next_ids, VACNIC_BAD_SHAPE, "sample_step: null operand");
  VCHECK(a->V >= 1 && a->V <= 65536, VACNIC_UNSUPPORTED, "sample_step: 1 <= V <= 65536, got %ld", (long)a->V);
  VCHECK(a->R >= 1 && a->R <= 0x7fffffffLL && a->ldl >= a->V, VACNIC_BAD_SHAPE, "sample_step: R >= 1 and ldl >= V");
  VCHECK(a->Lmax >= 2 && a->Lmax <= 0x7fffffffLL && a->cur_len >= 1 && a->cur_len < a->Lmax, VACNIC_BAD_SHAPE,
         "sample_step: cur_len %d outside [1, Lmax=%ld)", (int)a->cur_len, (long)a->Lmax);
  VCHECK(a->forced_token < a->V && a->no_repeat_ngram_size >= 0, VACNIC_BAD_SHAPE,
         "sample_step: forced token outside the vocabulary, or a negative n-gram size");
  VCHECK(a->n_bad >= 0 && a->n_bad <= VACNIC_BAD_WORDS_MAX, VACNIC_UNSUPPORTED, "sample_step: %d bad words, at most %d", (int)a->n_bad,
         (int)VACNIC_BAD_WORDS_MAX);
  VCHECK(a->n_bad == 0 || (a->bad_words && a->bad_len), VACNIC_BAD_SHAPE, "sample_step: bad-word table missing (null operand)");
  SampleP p;
  p.logits = a->logits; p.params = (const uint32_t*)a->params; p.seq = a->seq; p.done = a->done; p.next_ids = a->next_ids; p.logp = a->logp;
  p.kept = a->kept; p.thr = a->thr; p.mass = a->mass; p.u = a->u;
  p.ldl = (long)a->ldl; p.V = (int)a->V; p.Lmax = (int)a->Lmax; p.cur_len = a->cur_len; p.eos = a->eos; p.pad = a->pad;
  p.ngram = a->no_repeat_ngram_size; p.suppress_eos = a->suppress_eos; p.forced = a->forced_token;
  p.bad_words = a->bad_words; p.bad_len = a->bad_len; p.n_bad = a->n_bad;
  hipLaunchKernelGGL(sample_step_kernel, dim3((unsigned)a->R), dim3(ST), 0, (hipStream_t)stream, p);
  VLAUNCH_CHECK();
  return VACNIC_OK;
}
