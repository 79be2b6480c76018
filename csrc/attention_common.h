// Flash attention forward + backward on CDNA4 MFMA (NS-05; apex.contrib.multihead_attn core).
//
// Layout: q/k/v/o are [B, S, H, D] views with arbitrary batch / seq strides (so the packed
// QKV projection output [B, S, 3, H, D] is consumed in place, no split/transposes).
// D in {32, 64, 128, 256} (other head dims are zero-padded to the next one by the caller);
// bf16 / fp16 in, fp32 accumulate; optional causal mask, per-batch key lengths, an additive
// score bias (BIAS: [B|1, H|1, Sq|1, Sk] in the input dtype — attention masks as -inf, ALiBi /
// relative-position biases) and Philox dropout regenerated identically in backward.
//
// Files: this header holds what the kernels share (MFMA / LDS / cross-lane primitives, the dropout
// stream, the score-bias helpers, the tile constants); attention_fwd.h the forward kernel,
// attention_bwd.h the delta pre-pass, the dK/dV kernel and the dQ kernel; attention_impl.h the
// per-head-dim launchers. attention_d{32,64,128,256}.hip instantiate one head dim each (parallel
// compilation), attention.hip dispatches on the head dim, attention_f32.hip is the fp32-input unit.
//
// Forward (one workgroup = 4 wave64 = 128 query rows, 32 per wave; K/V streamed in 64-key
// tiles through LDS):
//   S^T = K . Q^T with v_mfma_f32_32x32x16 — the swapped product puts ONE query per lane
//   (16 keys in registers, the other 16 in lane^32), so row max / row sum need a single
//   cross-half exchange and the rescale factor is lane-local;
//   O^T += V^T . P^T reuses the S^T accumulator registers directly as the B operand
//   (k-order permuted to match, no LDS round trip for P); the V^T operand comes from the
//   row-major V tile with ds_read_b64_tr_b16 (hardware transpose read).
// Backward (one workgroup = 4 waves x 32 keys = 128 keys; loop over 32-query blocks):
//   S = Q.K^T and dP = dO.V^T with K, V rows held in registers; dV += P^T.dO and
//   dK += dS^T.Q use the accumulators as A operands with tr-read B operands from the
//   Q/dO tiles in LDS; dQ = dS.K goes through LDS (dS) when one workgroup holds every key
//   (Sk <= 128), and comes from a query-stationary kernel of its own beyond (attn_bwd_dq_kernel).
#pragma once
#include "common.h"
#include "fp8_pack.h"
#include "kernels.h"

#include <type_traits>

namespace apex {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename T> struct MfmaT;
template <> struct MfmaT<bf16> {
  using V8 = bf16x8;
  __device__ static __forceinline__ f32x16 mma(V8 a, V8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct MfmaT<f16> {
  using V8 = f16x8;
  __device__ static __forceinline__ f32x16 mma(V8 a, V8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

// 16x16x32 products (the backward's dQ tiles): lane l holds C[4 (l >> 4) + i][l & 15]
template <typename T> struct Mfma16T;
template <> struct Mfma16T<bf16> {
  __device__ static __forceinline__ f32x4 mma(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Mfma16T<f16> {
  __device__ static __forceinline__ f32x4 mma(f16x8 a, f16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// transposed LDS read: 4 rows x 16 cols block, lane i of each 16-lane group gets column i
__device__ __forceinline__ s16x4 lds_tr16(const void* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(p));
}

// LDS row strides (elements) of the 16-bit tiles, by how a tile is read. Bank model of
// MI355X_MICROARCH.md (LDS table): 16-byte row reads (ds_read_b128) are conflict-free at D + 8;
// transposed reads (ds_read_b64_tr_b16: 4 rows x 64 B per 32-lane group) need the rows 64 B apart
// modulo 256 B, i.e. D + 32; a tile read both ways is best at D + 8 (D = 64) / D + 24 (D >= 128),
// 2-way on the transposed reads. The uniform D + 8 made V's transposed reads 2-way (D = 64) and
// 4-way (D >= 128) conflicted: 22-48 % of all LDS cycles by rocprofv3 (profiles/r2_pmc_attn.json).
// (An XOR chunk swizzle makes the both-ways case conflict-free too, but its per-access address
// arithmetic cost registers — spills at D = 128 — in these VALU-bound loops.)
template <int D> constexpr int ld_rows() { return D + 8; }
template <int D> constexpr int ld_tr() { return D == 32 ? D : D + 32; }
template <int D> constexpr int ld_both() { return D >= 128 ? D + 24 : D + 8; }

// Workgroup barrier ordering LDS traffic only: the fences are restricted to the "local"
// address space, so outstanding global loads (register prefetches) are NOT drained at the
// barrier the way __syncthreads()'s full workgroup fence drains them.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Cross-lane exchanges without an LDS round trip (__shfl_xor lowers to ds_bpermute + a wait):
// the lane ^ 32 partner through gfx950's v_permlane32_swap, and sums over aligned groups of
// 4 / 8 / 16 lanes through DPP (quad_perm, row_half_mirror, row_mirror).
__device__ __forceinline__ uint32_t xor32_u(uint32_t v) {
  const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return (__lane_id() & 32) ? r[0] : r[1];
}
__device__ __forceinline__ float xor32_f(float v) { return __uint_as_float(xor32_u(__float_as_uint(v))); }
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int N>  // every lane of each aligned N-lane group ends with the group's sum
__device__ __forceinline__ float group_sum(float v) {
  static_assert(N == 1 || N == 2 || N == 4 || N == 8 || N == 16 || N == 32, "group size");
  if constexpr (N >= 2) v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2]: lane ^ 1
  if constexpr (N >= 4) v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1]: lane ^ 2
  if constexpr (N >= 8) v += dpp_f<0x141>(v);  // row_half_mirror: the other quad of the 8
  if constexpr (N >= 16) v += dpp_f<0x140>(v); // row_mirror: the other 8 of the row
  if constexpr (N >= 32) v += __shfl_xor(v, 16, 64);
  return v;
}

template <typename V8>
__device__ __forceinline__ V8 join4(s16x4 lo, s16x4 hi) {
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(V8, r);
}

// MFMA B operand read transposed from a row-major LDS tile (row stride ld): rows k0 .. k0 + 3 and
// k0 + 8 .. k0 + 11 of the 16 columns from c0 (k0 and c0 carry the lane's part, see lds_tr16)
template <typename V8, typename T>
__device__ __forceinline__ V8 tr_frag(const T* tile, int k0, int ld, int c0) {
  return join4<V8>(lds_tr16(tile + k0 * ld + c0), lds_tr16(tile + (k0 + 8) * ld + c0));
}

// Row (of the 32) that element i of a 32x32 accumulator holds in lane half hl: the key of a score
// in the query-per-lane kernels, the query in the key-per-lane ones (fp32 kernels alike).
// kappa(i): the same within the lane half's 16, e.g. the bit of a keep word shifted down by 4 hl
__device__ __forceinline__ int kappa(int i) { return (i & 3) + 8 * (i >> 2); }
__device__ __forceinline__ int kappa(int i, int hl) { return kappa(i) + 4 * hl; }

// grouped-query attention: the K/V head of query head h
__device__ __forceinline__ int kv_head(const AttnArgs& a, int h) { return a.kv_group > 1 ? h / a.kv_group : h; }

template <typename T, typename V8>
__device__ __forceinline__ V8 pack8(const float* x) {
  typedef T t8 __attribute__((ext_vector_type(8)));
  t8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (T)x[j];
  return __builtin_bit_cast(V8, r);
}

// Attention dropout keep bits: 8-bit uniforms (keep iff u8 >= thresh), 16 per (row, 16-key half of a
// 32-key block). Each (row, half) is one stream: ONE Philox4x32-7 call (counter offset + hl,
// subsequence bh * Sq + row) seeds a xorshift128 state, and every 32-key block then takes the
// stream's next four 32-bit words, in block order. Why not one Philox call per block and half: its
// 14 64-bit integer multiplies (quarter-rate v_mad_u64_u32) per call were ~30 % of the BERT-shape
// forward (fwd 72.7 us with p = 0.1 vs 56.1 at p = 0, b256 s128, tools/attn_bench.py); a xorshift128
// step is six full-rate shift/xor ops. Dropout masks need uniform, uncorrelated bytes, not
// cryptographic strength; the Philox seeding keeps streams of different rows / heads / launches
// independent, and tests/test_attention_gpu.py checks the keep rate and the mask's decorrelation.
// The four words are compared against the threshold four bytes at a time (SWAR: the carry out of
// u + (256 - thresh) in each byte is the keep bit — u & 0x7f.. plus the low 7 bits of the addend,
// then the majority of the three top bits), and the carries are shifted into the natural bit order:
// the returned 16 bits land at positions 4 hl + {0..3, 8..11, 16..19, 24..27}, i.e. bit k of the OR
// of both halves is key k of the block (random word j = k & 3 of half hl = (k >> 2) & 1, byte k >> 3).
struct DropStream {
  uint32_t x, y, z, w, thresh;
  __device__ __forceinline__ DropStream(uint64_t seed, uint64_t offset, uint32_t thr, int64_t bh, int64_t row,
                                        int hl, int64_t Sq) {
    Philox ph(seed, (uint64_t)(bh * Sq + row), offset + (uint64_t)hl);
    const uint4 r = ph.next();
    x = r.x;
    y = r.y;
    z = r.z;
    w = r.w | (uint32_t)((r.x | r.y | r.z | r.w) == 0u);  // xorshift128's state must not be all zero
    thresh = thr;
  }
  __device__ __forceinline__ uint32_t next() {
    const uint32_t t = x ^ (x << 11);
    x = y;
    y = z;
    z = w;
    w = w ^ (w >> 19) ^ t ^ (t >> 8);
    return w;
  }
  // keep decisions of the next random word's four bytes: bit 8b + 7 set iff byte b >= thresh
  __device__ __forceinline__ uint32_t next_keep4() {
    const uint32_t C = (256u - thresh) * 0x01010101u;
    const uint32_t C7 = C & 0x7f7f7f7fu;
    const uint32_t u = next();
    const uint32_t s7 = (u & 0x7f7f7f7fu) + C7;
    return ((u & C) | ((u | C) & s7)) & 0x80808080u;
  }
  // the next block's 16 keep bits of this half (bits 4 hl + {0-3, 8-11, 16-19, 24-27})
  __device__ __forceinline__ uint32_t half_bits(int hl) {
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) out |= next_keep4() >> (7 - j);  // bit 8b + 7 -> bit 8b + j
    return out << (4 * hl);
  }
  // half_bits plus the same decisions as byte masks for the P operand: byte b of bm[j] is 0xFF
  // iff element 4 b + j of the lane's 16 (key j + 8 b + 4 hl of the block) is kept. The forward
  // ANDs them into the packed bf16 P words (drop_pack): one v_perm + one v_and per pair of
  // probabilities instead of a bit test, compare and select per element on the fp32 values (which
  // also split the v_cvt_pk pairs: BERT-shape forward, 19 VALU instructions per score).
  __device__ __forceinline__ uint32_t half_masks(int hl, uint32_t (&bm)[4]) {
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t carry = next_keep4();
      out |= carry >> (7 - j);
      bm[j] = carry | (carry - (carry >> 7));  // 0x80 -> 0xFF per kept byte (no borrow across bytes)
    }
    return out << (4 * hl);
  }
};

// Dropout on 8 packed 16-bit probabilities (elements 8 s2 .. 8 s2 + 7 of a lane's 16, word w =
// elements 2w, 2w + 1): word w &= the byte masks of its two elements, gathered by v_perm_b32
// (bytes 0-1 <- byte b of bm[j], bytes 2-3 <- byte b of bm[j + 1], b = (8 s2 + 2w) >> 2)
template <typename V8>
__device__ __forceinline__ V8 drop_pack(V8 pf, const uint32_t (&bm)[4], int s2) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 w = __builtin_bit_cast(u32x4, pf);
#pragma unroll
  for (int ww = 0; ww < 4; ++ww) {
    const uint32_t b = 2 * s2 + (ww >> 1), j = 2 * (ww & 1);
    const uint32_t sel = b | (b << 8) | ((4 + b) << 16) | ((4 + b) << 24);
    w[ww] &= __builtin_amdgcn_perm(bm[j + 1], bm[j], sel);
  }
  return __builtin_bit_cast(V8, w);
}

// keep bits of block `blk` (bit k <-> key 32 blk + k) for one row, both halves (debug / test kernel)
__device__ __forceinline__ uint32_t drop_block_bits(uint64_t seed, uint64_t offset, uint32_t thresh, int64_t bh,
                                                    int64_t row, int64_t blk, int64_t Sq) {
  uint32_t out = 0;
  for (int hl = 0; hl < 2; ++hl) {
    DropStream st(seed, offset, thresh, bh, row, hl, Sq);
    uint32_t hb = 0;
    for (int64_t b = 0; b <= blk; ++b) hb = st.half_bits(hl);
    out |= hb;
  }
  return out;
}

// Additive score bias for this lane's query row and 4 consecutive keys key .. key+3 (8-byte load
// when all four are inside the row; keys >= Sk read 0 — they are masked anyway).
template <typename T>
__device__ __forceinline__ void bias4(const T* brow, int key, int Sk, float (&v)[4]) {
  if (key + 3 < Sk) {
    Pack<T, 4> pk = *reinterpret_cast<const Pack<T, 4>*>(brow + key);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = to_f(pk.v[e]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = key + e < Sk ? to_f(brow[key + e]) : 0.f;
  }
}

template <typename T>
__device__ __forceinline__ const T* bias_row(const AttnArgs& a, int b, int h, int q) {
  return (const T*)a.bias + b * a.bias_bs + h * a.bias_hs + (int64_t)min(q, a.Sq - 1) * a.bias_qs;
}

// forward and dQ kernels (query-stationary)
constexpr int kFwdWaves = 4;
constexpr int kFwdBQ = 32 * kFwdWaves;  // 128 query rows per workgroup
constexpr int kFwdKB = 64;              // keys per tile
// dK/dV kernel (key-stationary)
constexpr int kBwdWaves = 4;
constexpr int kBwdBK = 32 * kBwdWaves;  // 128 keys per workgroup
constexpr int kBwdBQ = 32;              // queries per inner step

}  // namespace apex
