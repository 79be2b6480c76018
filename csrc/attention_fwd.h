// Flash attention forward kernel (16-bit inputs). Overview and file map: attention_common.h.
#pragma once
#include "attention_common.h"

namespace apex {

// Waves per SIMD the forward is compiled for (= workgroups per CU: 4 waves, one per SIMD).
//   SHORT: 4 (128 VGPRs), which is what the variant exists for; with dropout 3, because at 4 the
//     keep-bit temporaries spill 4 VGPRs and it measured 10 % slower;
//   D = 256: 1 (the O accumulators alone are 128 registers);
//   double-buffered D <= 64 without dropout: 3 (GPT-2 s1024 104 -> 90 us); with dropout the
//     keep-bit temporaries spill at that budget, and D = 128 does not fit it: 2, as the two-barrier loop.
// Numbers: profiles/README.md ("Attention unit split").
constexpr int attn_fwd_waves_per_eu(int D, bool SHORT, bool DB, bool DROPOUT) {
  if (SHORT) return DROPOUT ? 3 : 4;
  if (D > 128) return 1;
  return DB && D <= 64 && !DROPOUT ? 3 : 2;
}

// SHORT (D = 64, Sk <= 128: BERT shape): the whole key range is staged into LDS once (36 KB)
// and no register copy of K/V is live during the math, which brings the kernel to 128 VGPRs:
// 4 workgroups (16 waves, 144 KB of LDS) per CU instead of 2 for a kernel that is one
// load -> math -> store pass per workgroup, so the other workgroups' loads hide the HBM latency.
// DB (long key ranges): K/V tiles double-buffered in LDS with ONE barrier per tile — tile kt + 1
// (in registers since the middle of tile kt - 1) is written to the other buffer in the middle of
// tile kt's math, right after the S products, and tile kt + 2's global loads are issued then
// (cdna_hip_programming.md T14 "async-STAGE split"); the single-buffer loop pays two barriers per
// tile (previous tile consumed / this tile staged).
// Which variant a launch takes: attn_fwd_loop in attention_impl.h.
template <typename T, int D, bool CAUSAL, bool DROPOUT, bool SHORT, bool BIAS, bool DB>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(attn_fwd_waves_per_eu(D, SHORT, DB, DROPOUT))))
attn_fwd_kernel(AttnArgs a) {
  static_assert(!SHORT || D == 64, "SHORT is the D = 64 single-pass variant");
  static_assert(!(SHORT && DB), "SHORT stages the whole key range once");
  using M = MfmaT<T>;
  using V8 = typename M::V8;
  constexpr int LDR = ld_rows<D>();  // K: row reads
  // V: transposed reads (SHORT keeps D + 8: the wider stride would take its two-tile LDS image to
  // 43 KB and the variant from 4 to 3 workgroups per CU)
  constexpr int LDV = SHORT ? ld_rows<D>() : ld_tr<D>();
  constexpr int NBUF = SHORT || DB ? 2 : 1;
  __shared__ __attribute__((aligned(16))) T lds_k[NBUF * kFwdKB * LDR];
  __shared__ __attribute__((aligned(16))) T lds_v[NBUF * kFwdKB * LDV];

  // wid through readfirstlane: wave-uniform in SGPRs, so tile-level conditions become scalar branches
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, hl = lane >> 5;
  const int bh = blockIdx.x;  // grid (B*H, query blocks): see attn_fwd_impl
  const int b = bh / a.H, h = bh % a.H;
  const int q0 = (CAUSAL ? gridDim.y - 1 - blockIdx.y : blockIdx.y) * kFwdBQ;
  const int qrow = q0 + 32 * wid + r;
  const int Sk = a.k_lens ? min(a.k_lens[b], a.Sk) : a.Sk;
  // BIAS: scores are taken to the natural domain s' = s * scale + bias, so the exp2 factor is log2(e)
  const float sl2 = BIAS ? kLog2e : a.scale_log2;

  const int hk = kv_head(a, h);
  const T* qp = (const T*)a.q + b * a.q_bs + h * a.q_hs;
  const T* kp = (const T*)a.k + b * a.k_bs + hk * a.k_hs;
  const T* vp = (const T*)a.v + b * a.v_bs + hk * a.v_hs;
  const T* brow = BIAS ? bias_row<T>(a, b, h, qrow) : nullptr;
  // fp8 codes of O: scale and the amax filter value read here, their latency under the main loop
  const float q8s = a.q8o ? a.q8_scale[0] : 0.f, q8seen = a.q8o ? f8_amax_seen(a.q8_amax) : 0.f;

  // Q^T fragments (B operand): lane (q=r, hl) holds Q[q][16s + 8hl .. +7]
  V8 qf[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    if (qrow < a.Sq) qf[s] = *(const V8*)(qp + (int64_t)qrow * a.q_ss + 16 * s + 8 * hl);
    else qf[s] = V8{};
  }

  f32x16 o[D / 32];
#pragma unroll
  for (int i = 0; i < D / 32; ++i) o[i] = f32x16{};
  float m = -INFINITY, l = 0.f;

  int kend = Sk;
  if (CAUSAL) kend = min(kend, q0 + kFwdBQ);
  const int ntiles = (kend + kFwdKB - 1) / kFwdKB;

  // tile loader: 64 x D elements, 16B chunks, CH chunks per thread
  constexpr int CPR = D / 8;               // chunks per row
  constexpr int CH = kFwdKB * CPR / 256;   // chunks per thread per tensor
  // K/V tiles of the tile TWO ahead are loaded into registers while the current tile computes
  // (two register sets, loop unrolled by two) at D <= 64; one ahead at D >= 128 (register budget)
  constexpr bool KV2 = D <= 64 && !DB;
  constexpr int AHEAD = KV2 ? 2 : 1;
  struct KV {
    uint4 k[CH], v[CH];
  };
  KV kva, kvb;
  // dropout: each lane draws the keep bits of its own 16 keys of every 32-key block in the
  // loop, in block order, from its (row, half) stream (DropStream::half_bits), and the two lane
  // halves' words are combined and stored for the backward kernels
  uint32_t* mrow =
      DROPOUT && qrow < a.Sq ? (uint32_t*)(a.dmask + ((int64_t)bh * a.Sq + qrow) * a.mask_words) : nullptr;
  DropStream dg(a.seed, a.offset, DROPOUT ? a.drop_thresh : 0u, bh, qrow, hl, a.Sq);
  // (gload / lstore are written out again in attn_bwd_dq_kernel: shared, they change the assembly)
  auto gload = [&](KV& R, int kt) {
    uint4 (&kreg)[CH] = R.k;
    uint4 (&vreg)[CH] = R.v;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int idx = threadIdx.x + 256 * c;
      const int row = idx / CPR, col = (idx % CPR) * 8;
      const int key = kt * kFwdKB + row;
      if (key < Sk) {
        kreg[c] = *(const uint4*)(kp + (int64_t)key * a.k_ss + col);
        vreg[c] = *(const uint4*)(vp + (int64_t)key * a.v_ss + col);
      } else {
        kreg[c] = make_uint4(0, 0, 0, 0);
        vreg[c] = make_uint4(0, 0, 0, 0);
      }
    }
  };
  auto lstore = [&](KV& R, const int rowoff) {
    uint4 (&kreg)[CH] = R.k;
    uint4 (&vreg)[CH] = R.v;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int idx = threadIdx.x + 256 * c;
      const int row = rowoff + idx / CPR, col = (idx % CPR) * 8;
      *(uint4*)(lds_k + row * LDR + col) = kreg[c];
      *(uint4*)(lds_v + row * LDV + col) = vreg[c];
    }
  };

  if (ntiles > 0) gload(kva, 0);
  if (KV2 && ntiles > 1) gload(kvb, 1);
  // math of key tile kt, read from LDS rows lr0 ..; mid() runs right after the S products (DB)
  auto compute = [&](const int kt, auto&& mid) {
    const int lr0 = SHORT ? kt * kFwdKB : DB ? (kt & 1) * kFwdKB : 0;
    uint32_t bm[2][4];
    if (DROPOUT) {
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
        const int blk = (kt * kFwdKB >> 5) + sb;
        const uint32_t hb = dg.half_masks(hl, bm[sb]);  // block blk's bits at 4 hl + {0-3, 8-11, ..}
        const uint32_t word = hb | xor32_u(hb);
        if (hl == 0 && mrow && blk * 32 < a.Sk) mrow[blk] = word;
      }
    }
    const int kb = kt * kFwdKB;

    // ---- S^T for two 32-key sub-blocks
    // all K fragments of the tile are read before the MFMA chain (one LDS latency per tile
    // instead of one per MFMA); D = 256 reads one sub-block at a time (register budget)
    f32x16 st[2];
    if constexpr (D <= 128) {
      V8 kf[2][D / 16];
#pragma unroll
      for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int s = 0; s < D / 16; ++s) kf[sb][s] = *(const V8*)(lds_k + (lr0 + 32 * sb + r) * LDR + 16 * s + 8 * hl);
      __builtin_amdgcn_sched_group_barrier(0x100, 2 * (D / 16), 0);  // DS reads first
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * (D / 16), 0);  // then the MFMAs
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
        st[sb] = f32x16{};
#pragma unroll
        for (int s = 0; s < D / 16; ++s) st[sb] = M::mma(kf[sb][s], qf[s], st[sb]);
      }
    } else {
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
        st[sb] = f32x16{};
#pragma unroll
        for (int s = 0; s < D / 16; ++s)
          st[sb] = M::mma(*(const V8*)(lds_k + (lr0 + 32 * sb + r) * LDR + 16 * s + 8 * hl), qf[s], st[sb]);
      }
    }
    mid();
    if constexpr (BIAS) {
      // element i = 4 g + e of sub-block sb <-> key kb + 32 sb + kappa(i, hl)
#pragma unroll
      for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float bv[4];
          bias4<T>(brow, kb + 32 * sb + 8 * g + 4 * hl, a.Sk, bv);
#pragma unroll
          for (int e = 0; e < 4; ++e) st[sb][4 * g + e] = fmaf(st[sb][4 * g + e], a.scale, bv[e]);
        }
    }
    // D = 64: the V^T fragments of the PV product are read now, their LDS latency hidden
    // behind the softmax (D = 128 would not fit in the register budget of 2 workgroups/CU)
    constexpr bool HOIST_V = D == 64;
    V8 vt[2][2][HOIST_V ? D / 32 : 1];
    if constexpr (HOIST_V) {
#pragma unroll
      for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int db = 0; db < D / 32; ++db) {
            const int k0 = lr0 + 32 * sb + 16 * s2 + 4 * hl + ((lane & 15) >> 2);
            const int c0 = 32 * db + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
            vt[sb][s2][db] = tr_frag<V8>(lds_v, k0, LDV, c0);
          }
    }
    // ---- mask (boundary tiles only) + running max on the RAW scores; the softmax scale is
    // folded into the exp2 argument (one FMA per element) and exp2 is the bare v_exp_f32
    // (no denormal range reduction: underflow to 0 is what softmax wants).
    const bool interior = (kb + kFwdKB <= Sk) && (!CAUSAL || kb + kFwdKB - 1 <= q0 + 32 * wid);
    if (!interior) {
      // keys valid for this lane's query: key < lim (one compare + select per element)
      const int lim = CAUSAL ? min(Sk, qrow + 1) : Sk;
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (kb + 32 * sb + kappa(i, hl) >= lim) st[sb][i] = -INFINITY;
        }
      }
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int i = 0; i < 16; ++i) tmax = fmaxf(tmax, st[sb][i]);
    tmax = fmaxf(tmax, xor32_f(tmax));
    const float mnew = fmaxf(m, tmax);
    const float muse = mnew == -INFINITY ? 0.f : mnew;
    const float alpha = __builtin_amdgcn_exp2f((m - muse) * sl2);
    const float mscaled = -muse * sl2;
    m = mnew;
    float psum = 0.f;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = __builtin_amdgcn_exp2f(fmaf(st[sb][i], sl2, mscaled));
        psum += p;
        // dropout is applied to the packed P operand below (drop_pack); the 1/(1-p) rescale once
        // in the epilogue
        st[sb][i] = p;
      }
    }
    l = l * alpha + psum;
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[db][i] *= alpha;
    // ---- O^T += V^T . P^T
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float pv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) pv[j] = st[sb][8 * s2 + j];
        V8 pf = pack8<T, V8>(pv);
        if constexpr (DROPOUT) pf = drop_pack(pf, bm[sb], s2);
        const int k0 = lr0 + 32 * sb + 16 * s2 + 4 * hl + ((lane & 15) >> 2);
#pragma unroll
        for (int db = 0; db < D / 32; ++db) {
          if constexpr (HOIST_V) {
            o[db] = M::mma(vt[sb][s2][db], pf, o[db]);
          } else {
            const int c0 = 32 * db + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
            o[db] = M::mma(tr_frag<V8>(lds_v, k0, LDV, c0), pf, o[db]);
          }
        }
      }
    }
  };
  auto nomid = [] {};
  auto tile = [&](KV& R, const int kt) {
    lds_barrier();  // previous tile fully consumed
    lstore(R, 0);
    lds_barrier();
    if (kt + AHEAD < ntiles) gload(R, kt + AHEAD);
    compute(kt, nomid);
  };
  if constexpr (SHORT) {
    // both (<= 2) tiles were loaded above: one LDS stage, then the math with no K/V registers live
    if (ntiles > 0) lstore(kva, 0);
    if (ntiles > 1) lstore(kvb, kFwdKB);
    lds_barrier();
    if (ntiles > 0) compute(0, nomid);
    if (ntiles > 1) compute(1, nomid);
  } else if constexpr (DB) {
    // tile 0 staged, tile 1 in registers; then per tile: barrier, S products, stage tile kt + 1
    // into the other buffer + issue tile kt + 2's loads, softmax, PV
    if (ntiles > 0) lstore(kva, 0);
    if (ntiles > 1) gload(kva, 1);
    for (int kt = 0; kt < ntiles; ++kt) {
      lds_barrier();  // tile kt's buffer complete; the other buffer's last readers (tile kt - 1) done
      compute(kt, [&] {
        if (kt + 1 < ntiles) {
          lstore(kva, ((kt + 1) & 1) * kFwdKB);
          if (kt + 2 < ntiles) gload(kva, kt + 2);
        }
      });
    }
  } else if constexpr (KV2) {
    for (int kt = 0; kt < ntiles; kt += 2) {
      tile(kva, kt);
      if (kt + 1 < ntiles) tile(kvb, kt + 1);
    }
  } else {
    for (int kt = 0; kt < ntiles; ++kt) tile(kva, kt);
  }
  // ---- epilogue
  const float ltot = l + xor32_f(l);
  float q8mx = 0.f;
  const float inv = ltot > 0.f ? (DROPOUT ? a.drop_scale : 1.f) / ltot : 0.f;
  // O rows packed to 16-bit: lane (r, hl) holds columns 32 db + 8 g + 4 hl .. + 3 of row qrow
  typedef T t4 __attribute__((ext_vector_type(4)));
  uint2 wv[D / 32][4];
#pragma unroll
  for (int db = 0; db < D / 32; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      t4 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = (T)(o[db][4 * g + e] * inv);
      wv[db][g] = __builtin_bit_cast(uint2, w);
    }
  // 16-byte row stores (cdna_hip_programming.md T21): for each column-group pair (g, g + 1) one
  // v_permlane32_swap per dword gives the lower half-wave columns 8 g .. 8 g + 7 of its row and the
  // upper half 8 g + 8 .. 8 g + 15 — half the store instructions of the 8-byte row-per-lane-pair
  // stores, same bytes (the store tail of a short-lived workgroup is issue-bound). The swaps run on
  // every lane, ahead of the row-validity branch. (attn_bwd_dq_kernel's epilogue does the same per
  // 32-column block; as one shared function it changes the assembly of both kernels.)
  uint4 wide[D / 32][2];
#pragma unroll
  for (int db = 0; db < D / 32; ++db)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const auto rx = __builtin_amdgcn_permlane32_swap(wv[db][2 * j].x, wv[db][2 * j + 1].x, false, false);
      const auto ry = __builtin_amdgcn_permlane32_swap(wv[db][2 * j].y, wv[db][2 * j + 1].y, false, false);
      wide[db][j] = make_uint4(rx[0], ry[0], rx[1], ry[1]);
    }
  if (qrow < a.Sq) {
    const int64_t ooff = b * a.o_bs + h * a.o_hs + (int64_t)qrow * a.o_ss;
    T* op = (T*)a.o + ooff;
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
      for (int j = 0; j < 2; ++j) *(uint4*)(op + 32 * db + 16 * j + 8 * hl) = wide[db][j];
    // Q8 (1: e4m3, 2: e5m2), switched on outside the store loop: fp8 codes of the stored
    // (rounded) values, the attention-out GEMM's operand, from the regrouped words: wide[db][j]
    // holds columns 32 db + 16 j + 8 hl .. + 7, so one more v_permlane32_swap per dword (the upper
    // half-wave's j = 0 codes for the lower half's j = 1 codes) gives the lower half columns
    // 32 db .. + 15 and the upper half 32 db + 16 .. + 31: one 16-byte code store per lane and
    // 32 columns (not two 8-byte stores: the store tail of these short workgroups is issue-bound)
    auto store_q8 = [&](auto Q8c) {
      constexpr int Q8 = decltype(Q8c)::value;
#pragma unroll
      for (int db = 0; db < D / 32; ++db) {
        uint32_t c[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          c[j][0] = f8_codes4<Q8 - 1, T>(wide[db][j].x, wide[db][j].y, q8s, q8mx);
          c[j][1] = f8_codes4<Q8 - 1, T>(wide[db][j].z, wide[db][j].w, q8s, q8mx);
        }
        const auto s0 = __builtin_amdgcn_permlane32_swap(c[0][0], c[1][0], false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(c[0][1], c[1][1], false, false);
        *(uint4*)(a.q8o + ooff + 32 * db + 16 * hl) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
      }
    };
    if (a.q8o) {
      if (a.q8_fmt == 0) store_q8(std::integral_constant<int, 1>{});
      else store_q8(std::integral_constant<int, 2>{});
    }
    if (hl == 0 && a.lse)
      a.lse[(int64_t)bh * a.Sq + qrow] = ltot > 0.f ? (m * sl2 + log2f(ltot)) * kLn2 : INFINITY;
  }
  if (a.q8o) f8_block_amax(q8mx, a.q8_amax, q8seen);  // every thread of the block reaches this
}

}  // namespace apex
