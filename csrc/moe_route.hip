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
//   moe_route_sigmoid_topk / _bwd   the sigmoid router (expert bias, group-limited top-k, scaled gate) in place
//                    of moe_route_topk / moe_route_bwd, on a work split of its own: see above its kernels
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

// ---------------------------------------------------------------------------
// Sigmoid router with an expert bias and group-limited top-k (moe_route_sigmoid_topk / _bwd).
//
// Work split, built for wide E: a token is held by a sub-wave of W <= 16 lanes, 64 / W tokens of a wave in flight,
// and lane j keeps the contiguous run of experts [j RUN, (j + 1) RUN) in registers (RUN = 4, 8 or 16, so that
// 16 RUN >= E; W narrows for small E until a lane holds one 16-byte vector: 4 fp32 or 8 16-bit values). Rows whose
// width is a multiple of the vector are read with 16-byte loads, other widths element by element. Contiguous runs
// make (lane, slot) order expert order, so ties fall to the lowest index with no index arithmetic.
//   group phase   a group that is a power-of-two number of whole runs: every lane takes the two largest keys of
//                 its run, log2(lanes per group) butterfly steps on the pair give the group's score, and a group
//                 is kept iff fewer than group_topk of the G broadcast scores beat it: no arg-max rounds. Groups
//                 that straddle runs (E = 200, G = 4) take a per-group top-2 over the whole sub-wave instead.
//   expert phase  topk rounds of log2(W) <= 4 butterfly steps on (key, index); a lane caches the best of its
//                 eligible slots and only the round's winner rescans its run. The gate's score s comes from the
//                 winner by one more shuffle (the key, s + bias, only selects).
//   gate / aux    from the sigmoids already in registers; per-expert sums go through s_psum as in the softmax
//                 kernel: tokens of a lane in pass order, sub-waves by butterfly, waves in order.
// The backward uses the same split; the chosen scores are recomputed from their logits (uniform over the
// sub-wave, no cross-lane traffic), the full row only for the aux loss.
constexpr int kSigMaxGroups = 16;

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// s[i] = sigmoid(logits[t, e0 + i]); 0 past E and on a dead row; NaN logits read as -inf (s = 0)
template <typename T, int RUN>
__device__ __forceinline__ void load_scores(const T* __restrict__ logits, int64_t t, bool live, int e0, int E, bool vec,
                                            float (&s)[RUN]) {
  constexpr int V = (16 / (int)sizeof(T)) < RUN ? (16 / (int)sizeof(T)) : RUN;
  float x[RUN];
#pragma unroll
  for (int i = 0; i < RUN; ++i) x[i] = -INFINITY;
  if (live) {
    if (vec) {
#pragma unroll
      for (int c = 0; c < RUN / V; ++c) {
        float tmp[V];
        if (e0 + c * V < E) {  // E % V == 0: a vector that starts inside the row ends inside it
          load_f<T, V>(logits + t * E + e0 + c * V, tmp);
#pragma unroll
          for (int i = 0; i < V; ++i) x[c * V + i] = tmp[i];
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < RUN; ++i)
        if (e0 + i < E) x[i] = to_f(logits[t * E + e0 + i]);
    }
  }
#pragma unroll
  for (int i = 0; i < RUN; ++i) s[i] = sigmoid_f(x[i] == x[i] ? x[i] : -INFINITY);
}

// the best key (ties to the lowest slot) among the slots of `avail`, its expert and its score
template <int RUN>
__device__ __forceinline__ void run_best(const float (&s)[RUN], const float (&b)[RUN], unsigned avail, int e0,
                                         float& bv, int& be, float& bs) {
  bv = -INFINITY, be = 0x7fffffff, bs = 0.f;
#pragma unroll
  for (int i = 0; i < RUN; ++i) {
    const float key = s[i] + b[i];
    if (((avail >> i) & 1u) && route_better(key, e0 + i, bv, be)) bv = key, be = e0 + i, bs = s[i];
  }
}

__device__ __forceinline__ void top2_merge(float& a1, float& a2, float o1, float o2) {
  a2 = fmaxf(fminf(a1, o1), fmaxf(a2, o2));
  a1 = fmaxf(a1, o1);
}

// The slots of `valid` whose group is kept: the group_topk groups with the largest sum of their two largest
// keys, ties to the lowest group. lpg > 0: a group is lpg whole runs (lanes); lpg == 0: any layout, gpack holds
// the group of slot i in bits [4 i, 4 i + 4).
template <int RUN>
__device__ __forceinline__ unsigned group_filter(const float (&s)[RUN], const float (&b)[RUN], unsigned valid,
                                                 unsigned long long gpack, int j, int W, int G, int gtopk, int lpg) {
  if (lpg > 0) {
    float a1 = -INFINITY, a2 = -INFINITY;
#pragma unroll
    for (int i = 0; i < RUN; ++i)
      if ((valid >> i) & 1u) top2_merge(a1, a2, s[i] + b[i], -INFINITY);
    for (int o = 1; o < lpg; o <<= 1) top2_merge(a1, a2, __shfl_xor(a1, o, kWave), __shfl_xor(a2, o, kWave));
    const float score = a1 + a2;
    const int myg = j / lpg;
    int beat = 0;
    for (int g = 0; g < G; ++g) {
      const float so = __shfl(score, g * lpg, W);
      beat += (so > score || (so == score && g < myg)) ? 1 : 0;
    }
    return beat < gtopk ? valid : 0u;
  }
  float sc[kSigMaxGroups];
#pragma unroll
  for (int g = 0; g < kSigMaxGroups; ++g) {
    sc[g] = -INFINITY;
    if (g < G) {
      float a1 = -INFINITY, a2 = -INFINITY;
#pragma unroll
      for (int i = 0; i < RUN; ++i)
        if (((valid >> i) & 1u) && (int)((gpack >> (4 * i)) & 15ull) == g) top2_merge(a1, a2, s[i] + b[i], -INFINITY);
      for (int o = W >> 1; o > 0; o >>= 1) top2_merge(a1, a2, __shfl_xor(a1, o, kWave), __shfl_xor(a2, o, kWave));
      sc[g] = a1 + a2;
    }
  }
  int beat[kSigMaxGroups];
#pragma unroll
  for (int g = 0; g < kSigMaxGroups; ++g) beat[g] = 0;
#pragma unroll
  for (int g = 0; g < kSigMaxGroups; ++g) {
#pragma unroll
    for (int h = g + 1; h < kSigMaxGroups; ++h) {
      if (h < G) {  // g < h: a tie goes to g
        const bool hw = sc[h] > sc[g];
        beat[g] += hw ? 1 : 0;
        beat[h] += hw ? 0 : 1;
      }
    }
  }
  unsigned keptg = 0u;
#pragma unroll
  for (int g = 0; g < kSigMaxGroups; ++g) keptg |= (g < G && beat[g] < gtopk) ? 1u << g : 0u;
  unsigned avail = 0u;
#pragma unroll
  for (int i = 0; i < RUN; ++i) avail |= ((keptg >> (int)((gpack >> (4 * i)) & 15ull)) & 1u) << i;
  return avail & valid;
}

// per lane: the bias of its run (0 without one; NaN reads as -inf), the mask of its slots below E and gpack
template <int RUN>
__device__ __forceinline__ void run_setup(const float* __restrict__ bias, int e0, int E, int G, float (&b)[RUN],
                                          unsigned& valid, unsigned long long& gpack) {
  valid = 0u, gpack = 0ull;
  const int S = G > 0 ? E / G : E;
#pragma unroll
  for (int i = 0; i < RUN; ++i) {
    b[i] = 0.f;
    if (e0 + i < E) {
      valid |= 1u << i;
      if (bias != nullptr) {
        const float x = bias[e0 + i];
        b[i] = x == x ? x : -INFINITY;
      }
      gpack |= (unsigned long long)((e0 + i) / S) << (4 * i);
    }
  }
}

template <typename T, int RUN>
__global__ void __launch_bounds__(kRouteTokens) moe_route_sigmoid_kernel(
    const T* __restrict__ logits, const float* __restrict__ bias, int Tn, int E, int topk, int W, int lw, int G,
    int gtopk, int lpg, float scale, bool vec, int R, int* __restrict__ ids, float* __restrict__ probs,
    int* __restrict__ rank, int* __restrict__ block_counts, float* __restrict__ block_psum,
    int* __restrict__ token_of_row, float* __restrict__ row_prob) {
  __shared__ int s_ids[kRouteTokens * kMoeMaxTopk];
  __shared__ int s_wcnt[4 * kRouteMaxE];
  __shared__ float s_psum[4 * kRouteMaxE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & (W - 1), sub = lane >> lw, tpp = 64 >> lw, e0 = j * RUN;
  const bool aux = block_psum != nullptr;
  fill_rows(token_of_row, row_prob, R);
  float b[RUN], pacc[RUN];
  unsigned valid;
  unsigned long long gpack;
  run_setup<RUN>(bias, e0, E, G, b, valid, gpack);
#pragma unroll
  for (int i = 0; i < RUN; ++i) pacc[i] = 0.f;
  for (int p = 0; p < W; ++p) {  // 64 tokens of the wave, tpp at a time
    const int tl = wave * 64 + p * tpp + sub;
    const int64_t t = (int64_t)blockIdx.x * kRouteTokens + tl;
    const bool live = t < Tn;
    float s[RUN];
    load_scores<T, RUN>(logits, t, live, e0, E, vec, s);
    unsigned avail = G > 0 ? group_filter<RUN>(s, b, valid, gpack, j, W, G, gtopk, lpg) : valid;
    float bv, bs, sum = 0.f;
    int be;
    run_best<RUN>(s, b, avail, e0, bv, be, bs);
    int idk[kMoeMaxTopk];
    float sk[kMoeMaxTopk];
#pragma unroll
    for (int k = 0; k < kMoeMaxTopk; ++k) {
      idk[k] = 0, sk[k] = 0.f;
      if (k < topk) {
        float wv = bv;
        int we = be;
        for (int o = W >> 1; o > 0; o >>= 1) {
          const float ov = __shfl_xor(wv, o, kWave);
          const int oe = __shfl_xor(we, o, kWave);
          if (route_better(ov, oe, wv, we)) wv = ov, we = oe;
        }
        we = clamp_id(we, E);  // topk eligible experts exist (checked on the host); the clamp makes it unconditional
        const int owner = we / RUN;
        sk[k] = __shfl(bs, owner, W);
        idk[k] = we;
        sum += sk[k];
        if (owner == j) {
          avail &= ~(1u << (we - e0));
          run_best<RUN>(s, b, avail, e0, bv, be, bs);
        }
      }
    }
    const float den = sum + 1e-20f;
#pragma unroll
    for (int k = 0; k < kMoeMaxTopk; ++k) {
      if (k < topk && (k & (W - 1)) == j) {
        s_ids[tl * topk + k] = live ? idk[k] : -1;
        if (live) {
          ids[t * topk + k] = idk[k];
          probs[t * topk + k] = topk > 1 ? scale * sk[k] / den : scale * sk[k];
        }
      }
    }
    if (aux) {  // dead rows hold s = 0
      float ls = 0.f;
#pragma unroll
      for (int i = 0; i < RUN; ++i) ls += s[i];
      const float dn = seg_sum(ls, W) + 1e-20f;
#pragma unroll
      for (int i = 0; i < RUN; ++i) pacc[i] += s[i] / dn;
    }
  }
  if (aux) {
#pragma unroll
    for (int i = 0; i < RUN; ++i) {
      for (int o = W; o < 64; o <<= 1) pacc[i] += __shfl_xor(pacc[i], o, kWave);
      if (sub == 0 && e0 + i < E) s_psum[wave * kRouteMaxE + e0 + i] = pacc[i];
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

template <typename T, int RUN>
__global__ void __launch_bounds__(kRouteTokens) moe_route_sigmoid_bwd_kernel(
    const T* __restrict__ logits, const int* __restrict__ ids, const float* __restrict__ probs,
    const float* __restrict__ dprobs, const int* __restrict__ tokens_per_expert, const float* __restrict__ d_aux,
    float aux_scale, float scale, int Tn, int E, int topk, int W, int lw, bool vec, T* __restrict__ dlogits) {
  constexpr int V = (16 / (int)sizeof(T)) < RUN ? (16 / (int)sizeof(T)) : RUN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & (W - 1), sub = lane >> lw, tpp = 64 >> lw, e0 = j * RUN;
  const bool aux = d_aux != nullptr;
  const float coef = aux ? d_aux[0] * aux_scale : 0.f;
  float c[RUN];
#pragma unroll
  for (int i = 0; i < RUN; ++i) c[i] = aux && e0 + i < E ? (float)tokens_per_expert[e0 + i] : 0.f;
  for (int p = 0; p < W; ++p) {
    const int64_t t = (int64_t)blockIdx.x * kRouteTokens + wave * 64 + p * tpp + sub;
    const bool live = t < Tn;
    float g[RUN];  // d loss / d s, then d loss / d logit
#pragma unroll
    for (int i = 0; i < RUN; ++i) g[i] = 0.f;
    if (dprobs != nullptr && live) {  // uniform over the sub-wave; the forward's sum, in its order
      float sk[kMoeMaxTopk], sum = 0.f, dot = 0.f;
#pragma unroll
      for (int k = 0; k < kMoeMaxTopk; ++k) {
        sk[k] = 0.f;
        if (k < topk) {
          const float x = to_f(logits[t * E + clamp_id(ids[t * topk + k], E)]);
          sk[k] = sigmoid_f(x == x ? x : -INFINITY);
          sum += sk[k];
          dot += probs[t * topk + k] * dprobs[t * topk + k];
        }
      }
      const float den = sum + 1e-20f;
#pragma unroll
      for (int k = 0; k < kMoeMaxTopk; ++k) {
        if (k < topk) {
          const float dp = scale * dprobs[t * topk + k];
          const float w = (topk > 1 ? (dp - dot) / den : dp) * (sk[k] * (1.f - sk[k]));
          const int slot = ids[t * topk + k] - e0;
#pragma unroll
          for (int i = 0; i < RUN; ++i)
            if (slot == i) g[i] = w;
        }
      }
    }
    if (aux) {
      float s[RUN];
      load_scores<T, RUN>(logits, t, live, e0, E, vec, s);
      float ls = 0.f;
#pragma unroll
      for (int i = 0; i < RUN; ++i) ls += s[i];
      const float dn = seg_sum(ls, W) + 1e-20f;
      float sc = 0.f;
#pragma unroll
      for (int i = 0; i < RUN; ++i) sc += s[i] / dn * c[i];
      sc = seg_sum(sc, W);
#pragma unroll
      for (int i = 0; i < RUN; ++i) g[i] += coef * (c[i] - sc) / dn * (s[i] * (1.f - s[i]));
    }
    if (live) {
      if (vec) {
#pragma unroll
        for (int q = 0; q < RUN / V; ++q) {
          float tmp[V];
#pragma unroll
          for (int i = 0; i < V; ++i) tmp[i] = g[q * V + i];
          if (e0 + q * V < E) store_f<T, V>(dlogits + t * E + e0 + q * V, tmp);
        }
      } else {
#pragma unroll
        for (int i = 0; i < RUN; ++i)
          if (e0 + i < E) dlogits[t * E + e0 + i] = from_f<T>(g[i]);
      }
    }
  }
}

// lanes per token W (a power of two <= 16), its log2 and the run per lane for E experts of element size esz
void sigmoid_split(int E, int esz, int& W, int& lw, int& run) {
  run = 16 / esz;
  while (16 * run < E) run <<= 1;
  W = 1, lw = 0;
  while (W * run < E) W <<= 1, ++lw;
}

// lanes per group when a group is a power-of-two number of whole runs, else 0 (the general group phase)
int sigmoid_lpg(int E, int G, int run) {
  if (G <= 0 || (E / G) % run != 0) return 0;
  const int l = E / G / run;
  return (l & (l - 1)) == 0 ? l : 0;
}

bool rows_vectorised(const void* p, int E, int esz) { return E % (16 / esz) == 0 && (uintptr_t)p % 16 == 0; }

#define ROUTE_DISPATCH_RUN(V, RUN, ...)                     \
  if (V == 4) { constexpr int RUN = 4; __VA_ARGS__; }       \
  else if (V == 8) { constexpr int RUN = 8; __VA_ARGS__; }  \
  else { constexpr int RUN = 16; __VA_ARGS__; }

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

bool moe_route_groups_ok(int64_t E, int64_t topk, int64_t num_groups, int64_t group_topk) {
  if (num_groups == 0) return group_topk == 0;
  return num_groups >= 1 && num_groups <= kSigMaxGroups && E % num_groups == 0 && E / num_groups >= 2 &&
         group_topk >= 1 && group_topk <= num_groups && topk <= group_topk * (E / num_groups);
}

int moe_route_sigmoid_topk(const MoeRouteArgs& a, int dt, hipStream_t s) {
  if (!route_args_ok(a) || !moe_route_supported(a.T, a.E, a.topk, dt) ||
      !moe_route_groups_ok(a.E, a.topk, a.num_groups, a.group_topk))
    return -2;
  const int esz = dt == kF32 ? 4 : 2;
  int W, lw, run;
  sigmoid_split(a.E, esz, W, lw, run);
  const int lpg = sigmoid_lpg(a.E, a.num_groups, run);
  const bool vec = rows_vectorised(a.logits, a.E, esz);
  const dim3 grid((a.T + kRouteTokens - 1) / kRouteTokens);
  APEX_DISPATCH_T(dt, T, ROUTE_DISPATCH_RUN(run, RUN, hipLaunchKernelGGL(
      (moe_route_sigmoid_kernel<T, RUN>), grid, dim3(kRouteTokens), 0, s, (const T*)a.logits, a.expert_bias, a.T, a.E,
      a.topk, W, lw, a.num_groups, a.group_topk, lpg, a.scaling, vec, a.R, a.expert_ids, a.probs, a.rank,
      a.block_counts, a.block_psum, a.token_of_row, a.row_prob)));
  return (int)hipGetLastError();
}

int moe_route_sigmoid_bwd(const MoeRouteArgs& a, const float* dprobs, const float* d_aux, void* dlogits, int dt,
                          hipStream_t s) {
  if (!route_args_ok(a) || !moe_route_supported(a.T, a.E, a.topk, dt)) return -2;
  const int esz = dt == kF32 ? 4 : 2;
  int W, lw, run;
  sigmoid_split(a.E, esz, W, lw, run);
  const bool vec = rows_vectorised(a.logits, a.E, esz) && (uintptr_t)dlogits % 16 == 0;
  const dim3 grid((a.T + kRouteTokens - 1) / kRouteTokens);
  APEX_DISPATCH_T(dt, T, ROUTE_DISPATCH_RUN(run, RUN, hipLaunchKernelGGL(
      (moe_route_sigmoid_bwd_kernel<T, RUN>), grid, dim3(kRouteTokens), 0, s, (const T*)a.logits, a.expert_ids,
      a.probs, dprobs, a.tokens_per_expert, d_aux, route_aux_scale(a), a.scaling, a.T, a.E, a.topk, W, lw, vec,
      (T*)dlogits)));
  return (int)hipGetLastError();
}

}  // namespace apex
