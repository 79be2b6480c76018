// Mixture-of-experts routing: from the router's logits [T, E] to the gate, the expert ids and the row maps
// of the expert-sorted layout (apex/ops/grouped.py), in three stream-ordered launches forward and one backward.
//
//   moe_route_topk   per token: top-k experts (ties to the lowest index, descending order), the gate (softmax over
//                    the chosen logits) and, for the load-balancing loss, the full softmax summed per expert over
//                    the block; per (t, k): its rank among the block's entries of the same expert, in flat
//                    t * topk + k order; per block: the count of every expert. Also presets token_of_row / row_prob.
//   moe_route_hist   the rank / count phase alone, from given expert ids (standalone moe_permute)
//   moe_route_scan   one workgroup: tokens_per_expert, offsets (counts rounded up to 64, running sum),
//                    block_base[b, e] = offsets[e] + the count of e in the blocks before b, and the aux loss
//   moe_route_place  dest[t, k] = block_base[t / 256, id] + rank[t, k]; token_of_row[dest] = t; row_prob[dest] = p
//   moe_route_bwd    dlogits [T, E] from dprobs and the aux loss's gradient, every element written
//
// Work split of topk and bwd: a workgroup owns 256 consecutive tokens, a wave 64 of them. Lanes run across
// experts, so the [T, E] reads are coalesced with no staging: for E >= 64 a wave holds one token at a time with
// VPL = 1, 2 or 4 values per lane (expert = lane + 64 i, the last ones ragged); for smaller E a wave is cut into
// segments of seg = pow2ceil(E) lanes and holds 64 / seg tokens at a time. Arg-max, max and sums are butterflies
// over a segment, so every lane of a segment ends with the same value. Top-k is topk rounds of arg-max on the
// pair (value, index) with a per-lane mask of taken values: -inf logits stay selectable and NaN is read as -inf,
// so every id is in [0, E) and a token never takes an expert twice.
//
// Rank phase: one lane per token. For each expert a wave ballot of "this token chose e" (a token chooses an
// expert at most once, so token order is flat order; given ids that repeat one take a ballot per multiplicity),
// the popcount of the lower lanes, and a 4-entry cross-wave prefix in LDS. moe_route_scan runs one lane per expert over the NB = ceil(T / 256) block rows (two passes of
// independent, coalesced loads: NB is 64 at T = 16384, so the lane-per-expert loop was kept over a
// wave-cooperative scan) and an LDS scan over the experts.
//
// No atomics, no cooperative launch, no workgroup waits on another: the row placement is bit-reproducible and
// equal to a stable sort of the flat ids. All math is fp32; every sum runs in a fixed order.
#include "common.h"
#include "kernels.h"

namespace apex {
namespace {

constexpr int kRouteTokens = 256;  // tokens per workgroup == threads per workgroup
constexpr int kRouteMaxE = 256;

__device__ __forceinline__ bool route_better(float av, int ae, float bv, int be) {
  return av > bv || (av == bv && ae < be);
}

__device__ __forceinline__ float seg_sum(float v, int seg) {
  for (int o = seg >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

__device__ __forceinline__ int clamp_id(int64_t id, int E) { return (int)(id < 0 ? 0 : (id >= E ? E - 1 : id)); }

// v[i] = logits[t, j + 64 i] as fp32; -inf past E, on a dead row and for NaN
template <typename T, int VPL>
__device__ __forceinline__ void load_logits(const T* __restrict__ logits, int64_t t, bool live, int j, int E,
                                            float (&v)[VPL]) {
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int e = j + 64 * i;
    float x = -INFINITY;
    if (live && e < E) x = to_f(logits[t * E + e]);
    v[i] = x == x ? x : -INFINITY;
  }
}

// ex[i] = exp(v[i] - m) (0 past E); returns their sum over the segment
template <int VPL>
__device__ __forceinline__ float softmax_terms(const float (&v)[VPL], float m, int seg, float (&ex)[VPL]) {
  float ls = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    ex[i] = expf(v[i] - m);
    ls += ex[i];
  }
  return seg_sum(ls, seg);
}

__device__ __forceinline__ void fill_rows(int* __restrict__ token_of_row, float* __restrict__ row_prob, int R) {
  for (int64_t i = (int64_t)blockIdx.x * kRouteTokens + threadIdx.x; i < R; i += (int64_t)gridDim.x * kRouteTokens) {
    token_of_row[i] = -1;
    if (row_prob != nullptr) row_prob[i] = 0.f;
  }
}

// One lane per token (thread tid owns token blockIdx.x * 256 + tid; id[k] < 0: no entry). Writes rank [T, topk] and
// block_counts [NB, E]; s_wcnt is [4][256] ints of LDS. Ends after a barrier, s_wcnt still valid.
__device__ __forceinline__ void rank_phase(const int (&id)[kMoeMaxTopk], int Tn, int E, int topk, int* s_wcnt,
                                           int* __restrict__ rank, int* __restrict__ block_counts) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long lower = (1ull << lane) - 1ull;
  int rk[kMoeMaxTopk];
#pragma unroll
  for (int k = 0; k < kMoeMaxTopk; ++k) rk[k] = 0;
  for (int e = 0; e < E; ++e) {
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kMoeMaxTopk; ++k) cnt += id[k] == e;
    const unsigned long long b = __ballot(cnt > 0);
    int r = __popcll(b & lower), tot = __popcll(b);
    if (__ballot(cnt > 1) != 0ull) {  // given ids that name an expert twice for one token (hist only)
      for (int m = 1; m < topk; ++m) {
        const unsigned long long bm = __ballot(cnt > m);
        r += __popcll(bm & lower);
        tot += __popcll(bm);
      }
    }
#pragma unroll
    for (int k = 0; k < kMoeMaxTopk; ++k)
      if (id[k] == e) rk[k] = r++;
    if (lane == 0) s_wcnt[wave * kRouteMaxE + e] = tot;
  }
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * kRouteTokens + tid;
  if (t < Tn) {
#pragma unroll
    for (int k = 0; k < kMoeMaxTopk; ++k) {
      if (k < topk) {
        const int e = clamp_id(id[k], E);
        int pre = 0;
#pragma unroll
        for (int w = 0; w < 3; ++w)
          if (w < wave) pre += s_wcnt[w * kRouteMaxE + e];
        rank[t * topk + k] = pre + rk[k];
      }
    }
  }
  if (tid < E)
    block_counts[(int64_t)blockIdx.x * E + tid] = s_wcnt[tid] + s_wcnt[kRouteMaxE + tid] + s_wcnt[2 * kRouteMaxE + tid] +
                                                  s_wcnt[3 * kRouteMaxE + tid];
}

template <typename T, int VPL>
__global__ void __launch_bounds__(kRouteTokens) moe_route_topk_kernel(
    const T* __restrict__ logits, int Tn, int E, int topk, int seg, int lseg, int R, int* __restrict__ ids,
    float* __restrict__ probs, int* __restrict__ rank, int* __restrict__ block_counts, float* __restrict__ block_psum,
    int* __restrict__ token_of_row, float* __restrict__ row_prob) {
  __shared__ int s_ids[kRouteTokens * kMoeMaxTopk];
  __shared__ int s_wcnt[4 * kRouteMaxE];
  __shared__ float s_psum[4 * kRouteMaxE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & (seg - 1), sub = lane >> lseg, tpp = 64 >> lseg;
  const bool aux = block_psum != nullptr;
  fill_rows(token_of_row, row_prob, R);
  float pacc[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) pacc[i] = 0.f;
  for (int p = 0; p < seg; ++p) {  // 64 tokens of the wave, tpp at a time
    const int tl = wave * 64 + p * tpp + sub;
    const int64_t t = (int64_t)blockIdx.x * kRouteTokens + tl;
    const bool live = t < Tn;
    float v[VPL];
    load_logits<T, VPL>(logits, t, live, j, E, v);
    unsigned taken = 0u;
    float m = 0.f, sum = 0.f, myv = 0.f;
    int mye = 0;
    for (int k = 0; k < topk; ++k) {
      float bv = -INFINITY;
      int be = 0x7fffffff;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int e = j + 64 * i;
        if (e < E && !((taken >> i) & 1u) && route_better(v[i], e, bv, be)) {
          bv = v[i];
          be = e;
        }
      }
      for (int o = seg >> 1; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, kWave);
        const int oe = __shfl_xor(be, o, kWave);
        if (route_better(ov, oe, bv, be)) {
          bv = ov;
          be = oe;
        }
      }
      be = clamp_id(be, E);  // topk <= E leaves a free expert in every round; the clamp makes it unconditional
      if ((be & (seg - 1)) == j) taken |= 1u << (be >> 6);
      if (k == 0) m = bv;
      sum += expf(bv - m);
      if (j == k) {
        myv = bv;
        mye = be;
      }
    }
    if (j < topk) {
      s_ids[tl * topk + j] = live ? mye : -1;
      if (live) {
        ids[t * topk + j] = mye;
        probs[t * topk + j] = expf(myv - m) / sum;
      }
    }
    if (aux) {  // m is the row's maximum: the first arg-max
      float ex[VPL];
      const float ls = softmax_terms<VPL>(v, m, seg, ex);
#pragma unroll
      for (int i = 0; i < VPL; ++i)
        if (live) pacc[i] += ex[i] / ls;
    }
  }
  if (aux) {  // tokens of a lane in pass order, the wave's segments by butterfly, the waves in order below
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      for (int o = seg; o < 64; o <<= 1) pacc[i] += __shfl_xor(pacc[i], o, kWave);
      if (sub == 0 && j + 64 * i < E) s_psum[wave * kRouteMaxE + j + 64 * i] = pacc[i];
    }
  }
  __syncthreads();
  int id[kMoeMaxTopk];
#pragma unroll
  for (int k = 0; k < kMoeMaxTopk; ++k) id[k] = k < topk ? s_ids[tid * topk + k] : -1;
  rank_phase(id, Tn, E, topk, s_wcnt, rank, block_counts);
  if (aux && tid < E)
    block_psum[(int64_t)blockIdx.x * E + tid] =
        ((s_psum[tid] + s_psum[kRouteMaxE + tid]) + s_psum[2 * kRouteMaxE + tid]) + s_psum[3 * kRouteMaxE + tid];
}

template <typename I>
__global__ void __launch_bounds__(kRouteTokens) moe_route_hist_kernel(const I* __restrict__ ids_in, int Tn, int E,
                                                                      int topk, int R, int* __restrict__ ids,
                                                                      int* __restrict__ rank,
                                                                      int* __restrict__ block_counts,
                                                                      int* __restrict__ token_of_row) {
  __shared__ int s_wcnt[4 * kRouteMaxE];
  fill_rows(token_of_row, nullptr, R);
  const int64_t t = (int64_t)blockIdx.x * kRouteTokens + threadIdx.x;
  int id[kMoeMaxTopk];
#pragma unroll
  for (int k = 0; k < kMoeMaxTopk; ++k) {
    id[k] = -1;
    if (k < topk && t < Tn) {
      id[k] = clamp_id((int64_t)ids_in[t * topk + k], E);
      ids[t * topk + k] = id[k];
    }
  }
  rank_phase(id, Tn, E, topk, s_wcnt, rank, block_counts);
}

__global__ void __launch_bounds__(kRouteTokens) moe_route_scan_kernel(
    const int* __restrict__ block_counts, const float* __restrict__ block_psum, int NB, int E, float aux_scale,
    int* __restrict__ tokens_per_expert, int* __restrict__ offsets, int* __restrict__ block_base,
    float* __restrict__ aux) {
  __shared__ int s_scan[kRouteTokens];
  __shared__ float red[4];
  const int e = threadIdx.x;
  int total = 0;
  float P = 0.f;
  if (e < E) {
#pragma unroll 8
    for (int b = 0; b < NB; ++b) total += block_counts[(int64_t)b * E + e];
    if (block_psum != nullptr) {
#pragma unroll 8
      for (int b = 0; b < NB; ++b) P += block_psum[(int64_t)b * E + e];
    }
  }
  const int padded = e < E ? (total + 63) / 64 * 64 : 0;
  s_scan[e] = padded;
  __syncthreads();
  for (int o = 1; o < kRouteTokens; o <<= 1) {  // inclusive scan over the experts
    const int add = e >= o ? s_scan[e - o] : 0;
    __syncthreads();
    s_scan[e] += add;
    __syncthreads();
  }
  if (e < E) {
    tokens_per_expert[e] = total;
    if (e == 0) offsets[0] = 0;
    offsets[e + 1] = s_scan[e];
    int run = s_scan[e] - padded;
#pragma unroll 8
    for (int b = 0; b < NB; ++b) {
      const int c = block_counts[(int64_t)b * E + e];
      block_base[(int64_t)b * E + e] = run;
      run += c;
    }
  }
  if (aux != nullptr) {
    const float s = block_sum(e < E ? (float)total * P : 0.f, red);
    if (e == 0) aux[0] = aux_scale * s;
  }
}

__global__ void __launch_bounds__(kRouteTokens) moe_route_place_kernel(
    const int* __restrict__ ids, const int* __restrict__ rank, const int* __restrict__ block_base,
    const float* __restrict__ probs, int n, int topk, int E, int R, int* __restrict__ dest,
    int* __restrict__ token_of_row, float* __restrict__ row_prob) {
  const int64_t i = (int64_t)blockIdx.x * kRouteTokens + threadIdx.x;
  if (i >= n) return;
  const int t = (int)(i / topk);
  const int d = block_base[(int64_t)(t / kRouteTokens) * E + clamp_id(ids[i], E)] + rank[i];
  dest[i] = d;
  if (d >= 0 && d < R) {
    token_of_row[d] = t;
    if (row_prob != nullptr) row_prob[d] = probs[i];
  }
}

template <typename T, int VPL>
__global__ void __launch_bounds__(kRouteTokens) moe_route_bwd_kernel(
    const T* __restrict__ logits, const int* __restrict__ ids, const float* __restrict__ probs,
    const float* __restrict__ dprobs, const int* __restrict__ tokens_per_expert, const float* __restrict__ d_aux,
    float aux_scale, int Tn, int E, int topk, int seg, int lseg, T* __restrict__ dlogits) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & (seg - 1), sub = lane >> lseg, tpp = 64 >> lseg;
  const bool aux = d_aux != nullptr;
  const float coef = aux ? d_aux[0] * aux_scale : 0.f;
  float c[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) c[i] = aux && j + 64 * i < E ? (float)tokens_per_expert[j + 64 * i] : 0.f;
  for (int p = 0; p < seg; ++p) {
    const int64_t t = (int64_t)blockIdx.x * kRouteTokens + wave * 64 + p * tpp + sub;
    const bool live = t < Tn;
    float g[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) g[i] = 0.f;
    if (dprobs != nullptr && live) {  // uniform over the segment; no cross-lane traffic inside
      float dot = 0.f;
      for (int k = 0; k < topk; ++k) dot += probs[t * topk + k] * dprobs[t * topk + k];
      for (int k = 0; k < topk; ++k) {
        const int id = ids[t * topk + k];
        const float w = probs[t * topk + k] * (dprobs[t * topk + k] - dot);
#pragma unroll
        for (int i = 0; i < VPL; ++i)
          if (id == j + 64 * i) g[i] += w;
      }
    }
    if (aux) {
      float v[VPL], ex[VPL];
      load_logits<T, VPL>(logits, t, live, j, E, v);
      float m = v[0];
#pragma unroll
      for (int i = 1; i < VPL; ++i) m = fmaxf(m, v[i]);
      for (int o = seg >> 1; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, kWave));
      const float ls = softmax_terms<VPL>(v, m, seg, ex);
      float sc = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        ex[i] = ex[i] / ls;
        sc += ex[i] * c[i];
      }
      sc = seg_sum(sc, seg);
#pragma unroll
      for (int i = 0; i < VPL; ++i) g[i] += coef * ex[i] * (c[i] - sc);
    }
#pragma unroll
    for (int i = 0; i < VPL; ++i)
      if (live && j + 64 * i < E) dlogits[t * E + j + 64 * i] = from_f<T>(g[i]);
  }
}

// segment width (lanes per token) and values per lane for E experts
void route_split(int E, int& seg, int& lseg, int& vpl) {
  seg = 1, lseg = 0;
  while (seg < E && seg < 64) seg <<= 1, ++lseg;
  vpl = E <= 64 ? 1 : (E <= 128 ? 2 : 4);
}

float route_aux_scale(const MoeRouteArgs& a) { return (float)((double)a.E / ((double)a.T * a.T * a.topk)); }

#define ROUTE_DISPATCH_VPL(V, VPL, ...)                \
  if (V == 1) { constexpr int VPL = 1; __VA_ARGS__; } \
  else if (V == 2) { constexpr int VPL = 2; __VA_ARGS__; } \
  else { constexpr int VPL = 4; __VA_ARGS__; }

}  // namespace

bool moe_route_supported(int64_t T, int64_t E, int64_t topk, int dt) {
  return (dt == kF32 || dt == kF16 || dt == kBF16) && topk >= 1 && topk <= kMoeMaxTopk && E >= topk &&
         E <= kRouteMaxE && T >= 1 && T * topk + 64 * E < (1ll << 31);
}

static bool route_args_ok(const MoeRouteArgs& a) {
  return moe_route_supported(a.T, a.E, a.topk, kF32) &&
         a.R == ((int64_t)a.T * a.topk + 63) / 64 * 64 + 64 * (int64_t)a.E;
}

int moe_route_topk(const MoeRouteArgs& a, int dt, hipStream_t s) {
  if (!route_args_ok(a) || !moe_route_supported(a.T, a.E, a.topk, dt)) return -2;
  int seg, lseg, vpl;
  route_split(a.E, seg, lseg, vpl);
  const dim3 grid((a.T + kRouteTokens - 1) / kRouteTokens);
  APEX_DISPATCH_T(dt, T, ROUTE_DISPATCH_VPL(vpl, VPL, hipLaunchKernelGGL(
      (moe_route_topk_kernel<T, VPL>), grid, dim3(kRouteTokens), 0, s, (const T*)a.logits, a.T, a.E, a.topk, seg, lseg,
      a.R, a.expert_ids, a.probs, a.rank, a.block_counts, a.block_psum, a.token_of_row, a.row_prob)));
  return (int)hipGetLastError();
}

int moe_route_hist(const MoeRouteArgs& a, bool ids_i64, hipStream_t s) {
  if (!route_args_ok(a)) return -2;
  const dim3 grid((a.T + kRouteTokens - 1) / kRouteTokens);
  if (ids_i64)
    hipLaunchKernelGGL((moe_route_hist_kernel<int64_t>), grid, dim3(kRouteTokens), 0, s, (const int64_t*)a.ids_in, a.T,
                       a.E, a.topk, a.R, a.expert_ids, a.rank, a.block_counts, a.token_of_row);
  else
    hipLaunchKernelGGL((moe_route_hist_kernel<int>), grid, dim3(kRouteTokens), 0, s, (const int*)a.ids_in, a.T, a.E,
                       a.topk, a.R, a.expert_ids, a.rank, a.block_counts, a.token_of_row);
  return (int)hipGetLastError();
}

int moe_route_scan(const MoeRouteArgs& a, hipStream_t s) {
  if (!route_args_ok(a) || (a.block_psum != nullptr) != (a.aux != nullptr)) return -2;
  hipLaunchKernelGGL(moe_route_scan_kernel, dim3(1), dim3(kRouteTokens), 0, s, a.block_counts, a.block_psum,
                     (a.T + kRouteTokens - 1) / kRouteTokens, a.E, route_aux_scale(a), a.tokens_per_expert, a.offsets,
                     a.block_base, a.aux);
  return (int)hipGetLastError();
}

int moe_route_place(const MoeRouteArgs& a, hipStream_t s) {
  if (!route_args_ok(a)) return -2;
  const int n = a.T * a.topk;
  hipLaunchKernelGGL(moe_route_place_kernel, dim3((n + kRouteTokens - 1) / kRouteTokens), dim3(kRouteTokens), 0, s,
                     a.expert_ids, a.rank, a.block_base, a.probs, n, a.topk, a.E, a.R, a.dest, a.token_of_row,
                     a.row_prob);
  return (int)hipGetLastError();
}

int moe_route_bwd(const MoeRouteArgs& a, const float* dprobs, const float* d_aux, void* dlogits, int dt,
                  hipStream_t s) {
  if (!route_args_ok(a) || !moe_route_supported(a.T, a.E, a.topk, dt)) return -2;
  int seg, lseg, vpl;
  route_split(a.E, seg, lseg, vpl);
  const dim3 grid((a.T + kRouteTokens - 1) / kRouteTokens);
  APEX_DISPATCH_T(dt, T, ROUTE_DISPATCH_VPL(vpl, VPL, hipLaunchKernelGGL(
      (moe_route_bwd_kernel<T, VPL>), grid, dim3(kRouteTokens), 0, s, (const T*)a.logits, a.expert_ids, a.probs, dprobs,
      a.tokens_per_expert, d_aux, route_aux_scale(a), a.T, a.E, a.topk, seg, lseg, (T*)dlogits)));
  return (int)hipGetLastError();
}

}  // namespace apex
