// Flash attention backward kernels (16-bit inputs; the delta pre-pass also serves the fp32 unit).
// Overview and file map: attention_common.h.
#pragma once
#include "attention_common.h"

namespace apex {

// delta = rowsum(dO * O) per query row, once, for the two-kernel backward: computed inside the
// dK/dV kernel it would be redone by every workgroup of a query block (a third 32 x D tile load,
// its unpack and a shuffle reduction per step, Sk / 128 times per row).
template <typename T, int D>
__global__ void __launch_bounds__(256) attn_bwd_delta_kernel(AttnArgs a, const void* dout, float* delta) {
  constexpr int CPR = D / 8;  // 16-byte chunks per row (4..32 lanes, a power of two)
  const int bh = blockIdx.y;
  const int b = bh / a.H, h = bh % a.H;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int q = idx / CPR, col = (idx % CPR) * 8;
  float part = 0.f;
  if (q < a.Sq) {
    float ov[8], dov[8];
    load_f<T, 8>((const T*)a.o + b * a.o_bs + h * a.o_hs + (int64_t)q * a.o_ss + col, ov);
    load_f<T, 8>((const T*)dout + b * a.do_bs + h * a.do_hs + (int64_t)q * a.do_ss + col, dov);
#pragma unroll
    for (int e = 0; e < 8; ++e) part += ov[e] * dov[e];
  }
  part = group_sum<CPR>(part);
  if (q < a.Sq && (idx % CPR) == 0) delta[(int64_t)bh * a.Sq + q] = part;
}

// DSUM adds up the gradients AS STORED. For fp16 the compiler (fp-contract=fast) otherwise forms the
// two copies of (T)(x * mul) differently: the stored one as v_mul_f32 + v_cvt_pk_f16_f32 (the product
// rounded to fp32, then to fp16), the summed one as v_fma_mixlo_f16 (the exact product rounded to fp16
// once). Where the product lies next to an fp16 rounding midpoint they are one fp16 ulp apart, and the
// column sum is off by that ulp (2**-11 for an element in [0.5, 1): tests/test_attn_numerics_gpu.py).
// The fp32 product is made opaque here, so one conversion serves both. (bf16 has no mixed-precision
// FMA: both copies already come from the same fp32 product.)
template <typename T, bool DSUM>
__device__ __forceinline__ T stored_product(float x, float mul) {
  float p = x * mul;
  if constexpr (DSUM && std::is_same_v<T, f16>) asm volatile("" : "+v"(p));
  return (T)p;
}

// DQ = true (Sk <= 128: the workgroup holds every key, so it is the sole owner of dQ for its
// query rows and writes it directly; delta is computed here from O). DQ = false (longer key
// ranges): dK/dV only, delta read from attn_bwd_delta_kernel's output, and attn_bwd_dq_kernel
// computes dQ from a query-stationary loop (no cross-workgroup fp32 atomics; see the kernel below).
template <typename T, int D, bool CAUSAL, bool DROPOUT, bool DSUM, bool DQ, bool BIAS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D <= 64 ? 2 : 1, D <= 64 ? 2 : 1))) attn_bwd_kernel(AttnArgs a, const void* dout, const float* delta_in,
                                                         void* dk_out, void* dv_out) {
  using M = MfmaT<T>;
  using V8 = typename M::V8;
  constexpr int LDR = D + 8;          // dK / dV emit staging in lds_k (row reads)
  constexpr int LDQ = ld_both<D>();  // Q / dO: row and transposed reads
  // dS^T [key][q] (bf16): each lane writes its 16 query values of one key as 4 x ds_write_b64 (4
  // consecutive queries each; row stride 36 elements = 18 dwords: the 16 rows of a lane group land
  // on distinct bank pairs), the dQ product reads it back with ds_read_b64_tr_b16 (a [q][key] image
  // costs 16 ds_write_b16 per lane and step).
  // D = 64: dS^T unpadded, 8-byte piece c of key row k at c ^ ((k >> 1) & 7): the ds_write_b64 stores
  // and the dQ product's transposed reads both conflict-free (tools/lds_banks.py; 36: reads 2-way)
  constexpr bool DSW = D == 64;
  constexpr int LDT = DSW ? kBwdBQ : kBwdBQ + 4;
  auto dso = [](int row, int col) -> int {
    if constexpr (DSW) return row * LDT + (col ^ (((row >> 1) & 7) << 2));
    else return row * LDT + col;
  };
  // K^T row stride (elements); K^T shares lds_k. 144: the dQ product's 16-byte K^T row reads are
  // conflict-free (136: 2-way; tools/lds_banks.py)
  constexpr int KT_LD = kBwdBK + 16;
  constexpr int LDSK = D * KT_LD > kBwdBK * LDR ? D * KT_LD : kBwdBK * LDR;
  __shared__ __attribute__((aligned(16))) T lds_q[kBwdBQ * LDQ];
  __shared__ __attribute__((aligned(16))) T lds_do[kBwdBQ * LDQ];
  __shared__ __attribute__((aligned(16))) T lds_k[LDSK];
  __shared__ __attribute__((aligned(16))) T lds_ds[kBwdBK * LDT];
  __shared__ __attribute__((aligned(16))) float lds_lse[kBwdBQ], lds_delta[kBwdBQ];
  __shared__ __attribute__((aligned(16))) uint32_t lds_mask[4 * kBwdBQ];  // [wave's 32-key block][q]: bit k <-> key 32 wid + k

  // wid through readfirstlane: wave-uniform in SGPRs, so tile-level conditions become scalar branches
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, hl = lane >> 5;
  const int bh = blockIdx.x;  // grid (B*H, key blocks): key block 0 (the most queries when causal) first
  const int b = bh / a.H, h = bh % a.H;
  const int k0 = blockIdx.y * kBwdBK;
  const int Sk = a.k_lens ? min(a.k_lens[b], a.Sk) : a.Sk;
  const int mykey = k0 + 32 * wid + r;  // key row this lane holds as K/V operand

  const T* qp = (const T*)a.q + b * a.q_bs + h * a.q_hs;
  const int hk = kv_head(a, h);
  const T* kp = (const T*)a.k + b * a.k_bs + hk * a.k_hs;
  const T* vp = (const T*)a.v + b * a.v_bs + hk * a.v_hs;
  const T* dop = (const T*)dout + b * a.do_bs + h * a.do_hs;
  const T* op = (const T*)a.o + b * a.o_bs + h * a.o_hs;
  const float* lsep = a.lse + (int64_t)bh * a.Sq;
  const float* dlp = DQ ? nullptr : delta_in + (int64_t)bh * a.Sq;
  // BIAS: this lane's key column of the bias, bcol[q * bias_qs]
  const T* bcol = BIAS ? (const T*)a.bias + b * a.bias_bs + h * a.bias_hs + min(mykey, a.Sk - 1) : nullptr;

  // accumulators: dK, dV  [key x dim]: C rows = keys (regs), cols = dim (lanes)
  f32x16 dk[D / 32], dv[D / 32];
#pragma unroll
  for (int i = 0; i < D / 32; ++i) {
    dk[i] = f32x16{};
    dv[i] = f32x16{};
  }

  int qstart = 0;
  if (CAUSAL) qstart = (k0 / kBwdBQ) * kBwdBQ;
  const int nq = a.Sq;
  const float rkeep = a.drop_scale;

  // Q / dO / O tiles (32 x D), lse and the dropout words of the query block TWO steps ahead
  // are loaded into registers while the current block computes (two register sets, the loop
  // unrolled by two, so every global load has two steps of compute to land in); the barriers
  // below only wait for LDS traffic so these global loads stay in flight across them.
  constexpr int CPR = D / 8;
  constexpr int NCHK = kBwdBQ * CPR;                // 16-byte chunks per 32-row tile
  constexpr int NLD = NCHK >= 256 ? NCHK / 256 : 1;  // per thread (D = 32: half the threads)
  struct Pf {
    uint4 q[NLD], d[NLD], o[DQ ? NLD : 1];
    float lse, dl;
    uint32_t mask;
  };
  // two register sets where they fit (dK/dV-only kernel at D = 64); one set (prefetch one step
  // ahead) for the fused single-key-block kernel and D = 128, which would spill
  constexpr bool DEPTH2 = !DQ && D <= 64;
  constexpr int AHEAD = DEPTH2 ? 2 : 1;
  Pf pfa, pfb;
  auto fetch = [&](Pf& P, int qb) {
    uint4 (&pf_q)[NLD] = P.q;
    uint4 (&pf_do)[NLD] = P.d;
    float& pf_lse = P.lse;
    uint32_t& pf_mask = P.mask;
    pf_lse = INFINITY;
    pf_mask = 0u;
    // block base pointers are wave-uniform (scalar 64-bit math); the per-lane part is a 32-bit
    // offset (row < 32 rows of one block) that the compiler hoists out of the loop
    const T* qbase = qp + (int64_t)qb * a.q_ss;
    const T* dbase = dop + (int64_t)qb * a.do_ss;
#pragma unroll
    for (int c = 0; c < NLD; ++c) {
      const int idx = threadIdx.x + 256 * c;
      const int row = idx / CPR, col = (idx % CPR) * 8;
      const int q = qb + row;
      if (q < nq && idx < NCHK) {
        pf_q[c] = *(const uint4*)(qbase + (row * (int)a.q_ss + col));
        pf_do[c] = *(const uint4*)(dbase + (row * (int)a.do_ss + col));
        if constexpr (DQ) P.o[c] = *(const uint4*)(op + (int64_t)q * a.o_ss + col);
      } else {
        pf_q[c] = pf_do[c] = make_uint4(0, 0, 0, 0);
        if constexpr (DQ) P.o[c] = make_uint4(0, 0, 0, 0);
      }
    }
    // raw values only: any arithmetic on a loaded value here would make the compiler wait for
    // the whole prefetch (s_waitcnt vmcnt(0)) instead of letting it land during the next step
    if (threadIdx.x < kBwdBQ) {
      const int q = qb + threadIdx.x;
      if (q < nq) pf_lse = lsep[q];  // natural log; x log2(e) at staging
    }
    if (!DQ && threadIdx.x >= 128 && threadIdx.x < 128 + kBwdBQ) {
      const int q = qb + threadIdx.x - 128;
      P.dl = q < nq ? dlp[q] : 0.f;
    }
    if (DROPOUT && threadIdx.x < 4 * kBwdBQ) {
      // dropout words written by the forward: one per (query, 32-key block), bit k <-> key k
      const int qi = threadIdx.x & (kBwdBQ - 1), w = threadIdx.x / kBwdBQ;
      const int q = qb + qi, blk = (k0 >> 5) + w;
      if (q < nq && blk * 32 < a.Sk) pf_mask = ((const uint32_t*)(a.dmask + ((int64_t)bh * a.Sq + q) * a.mask_words))[blk];
    }
  };
  V8 kf[D / 16], vf[D / 16];
  auto load_kv = [&]() {
    // K and V rows for this wave's 32 keys as B operands: lane (key=r, hl) holds X[key][16s+8hl..]
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      if (mykey < Sk) {
        kf[s] = *(const V8*)(kp + (int64_t)mykey * a.k_ss + 16 * s + 8 * hl);
        vf[s] = *(const V8*)(vp + (int64_t)mykey * a.v_ss + 16 * s + 8 * hl);
      } else {
        kf[s] = V8{};
        vf[s] = V8{};
      }
    }
    // whole K block to LDS transposed, K^T [D][KT_LD] (the A operand of dQ^T = K^T . dS^T, read as
    // 16-byte rows), written once per workgroup from the K rows just loaded as B operands (kf: key
    // mykey, dims 16s + 8hl .. +7; zero past Sk): each 2-byte store instruction writes one dim row, 32
    // consecutive keys per half-wave — conflict-free, and no second global read of K. (Staging it
    // from a fresh 16-byte-per-lane load of K, 8 dims x 8 keys per half-wave, has 8-way conflicts,
    // half of the kernel's conflict cycles; a conflict-free re-load needs strided global loads.)
    if constexpr (DQ) {
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        const T* e = (const T*)&kf[s];
#pragma unroll
        for (int j = 0; j < 8; ++j) lds_k[(16 * s + 8 * hl + j) * KT_LD + 32 * wid + r] = e[j];
      }
    }
  };
  // D <= 64: the K/V loads are issued after the first query-block fetch, so both latencies
  // overlap (at D >= 128 that order spills registers)
  if (D >= 128) load_kv();
  if (qstart < nq) fetch(pfa, qstart);
  if (DEPTH2 && qstart + kBwdBQ < nq) fetch(pfb, qstart + kBwdBQ);
  if (D < 128) load_kv();

  float dqcs[D / 32][4] = {};  // DSUM: this lane's dq dims (see the dQ section) summed over queries
  // fp8 producer-side codes of dq / dk / dv (AttnArgs::q8dq..): running max|value| of this lane
  float q8mx = 0.f;
  const float q8s = a.q8dq ? a.q8_scale[0] : 0.f, q8seen = a.q8dq ? f8_amax_seen(a.q8_amax) : 0.f;
  auto body = [&](Pf& P, const int qb) {
    uint4 (&pf_q)[NLD] = P.q;
    uint4 (&pf_do)[NLD] = P.d;
    if constexpr (D >= 128) {
      // keep dK / dV in AGPRs across the step (else the allocator parks two of them in VGPRs while
      // the S / dP products use their AGPRs: 64 accvgpr moves per step)
#pragma unroll
      for (int i = 0; i < D / 32; ++i) asm volatile("" : "+a"(dk[i]), "+a"(dv[i]));
    }
    lds_barrier();
    // stage the prefetched tiles; delta = rowsum(dO * O) is computed here from O
    // (CPR consecutive threads own one row -> xor-shuffle reduce), no separate pass.
#pragma unroll
    for (int c = 0; c < NLD; ++c) {
      const int idx = threadIdx.x + 256 * c;
      if (NCHK < 256 && idx >= NCHK) break;  // (wave-uniform: D = 32 leaves waves 2, 3 out)
      const int row = idx / CPR, col = (idx % CPR) * 8;
      if constexpr (DQ) {
        float ov[8], dov[8];
        load_f<T, 8>((const T*)&P.o[c], ov);
        load_f<T, 8>((const T*)&pf_do[c], dov);
        float part = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) part += ov[e] * dov[e];
        part = group_sum<CPR>(part);
        if ((idx % CPR) == 0) lds_delta[row] = part;
      }
      *(uint4*)(lds_q + row * LDQ + col) = pf_q[c];
      *(uint4*)(lds_do + row * LDQ + col) = pf_do[c];
    }
    if (threadIdx.x < kBwdBQ) lds_lse[threadIdx.x] = P.lse * kLog2e;  // +inf stays +inf
    if (!DQ && threadIdx.x >= 128 && threadIdx.x < 128 + kBwdBQ) lds_delta[threadIdx.x - 128] = P.dl;
    if (DROPOUT && threadIdx.x < 4 * kBwdBQ) lds_mask[threadIdx.x] = P.mask;
    if (qb + AHEAD * kBwdBQ < nq) fetch(P, qb + AHEAD * kBwdBQ);
    lds_barrier();

    // D >= 128 (one wave per SIMD): lse / delta / dropout words of this lane's 16 query rows
    // (8g + 4hl + e, e = 0..3) as 16-byte LDS reads issued ahead of the S / dP products, so their
    // latency hides behind the MFMAs (a scalar read + wait per element exposed ~16 LDS round trips
    // per step with no partner wave to cover them). D <= 64 runs two waves per SIMD and has no
    // 48 spare VGPRs: it reads the scalars in the elementwise loop.
    constexpr bool VROWS = D >= 128;
    f32x4 lse4[4], del4[4];
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 msk4[4];
    if constexpr (VROWS) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        lse4[g] = *(const f32x4*)(lds_lse + 8 * g + 4 * hl);
        del4[g] = *(const f32x4*)(lds_delta + 8 * g + 4 * hl);
        if (DROPOUT) msk4[g] = *(const u32x4*)(lds_mask + wid * kBwdBQ + 8 * g + 4 * hl);
      }
    }

    // S = Q . K^T  [32 q x 32 keys]: A = Q rows (LDS), B = K rows (regs)
    f32x16 sacc = f32x16{}, dpacc = f32x16{};
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      const V8 qa = *(const V8*)(lds_q + r * LDQ + 16 * s + 8 * hl);
      const V8 da = *(const V8*)(lds_do + r * LDQ + 16 * s + 8 * hl);
      sacc = M::mma(qa, kf[s], sacc);
      dpacc = M::mma(da, vf[s], dpacc);
    }
    // element i: q = qb + kappa(i, hl), key = mykey.
    // pd = P * keep (the 1/(1-p) factor of dV is applied once, in the epilogue),
    // ds = P * (dP * keep / (1-p) - delta) (the softmax scale of dK / dQ likewise).
    float pd[16], ds[16];
    const bool interior = (k0 + 32 * wid + 31 < Sk) && (qb + kBwdBQ <= nq) && (!CAUSAL || k0 + 32 * wid + 31 <= qb);
    // exp2 is the bare v_exp_f32 (no denormal range reduction). One wave-uniform branch picks the
    // boundary variant for the whole tile (a per-element branch split the section into 16 blocks
    // the scheduler could not interleave).
    auto elementwise = [&](auto bound_tag) {
      constexpr bool BOUND = decltype(bound_tag)::value;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        // this lane's 4 query rows 8g + 4hl + e of lse / delta / dropout words: one 16-byte LDS read
        // each (12 per step at D <= 64 instead of 48 scalar ds_read_b32)
        f32x4 lg4, dg4;
        u32x4 mg4;
        if constexpr (VROWS) {
          lg4 = lse4[g];
          dg4 = del4[g];
          if constexpr (DROPOUT) mg4 = msk4[g];
        } else {
          lg4 = *(const f32x4*)(lds_lse + 8 * g + 4 * hl);
          dg4 = *(const f32x4*)(lds_delta + 8 * g + 4 * hl);
          if constexpr (DROPOUT) mg4 = *(const u32x4*)(lds_mask + wid * kBwdBQ + 8 * g + 4 * hl);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g + e;
          const int qi = 8 * g + 4 * hl + e;
          float lterm = -lg4[e];
          if constexpr (BIAS) {
            const int q = qb + qi;
            if (q < nq && mykey < Sk) lterm = fmaf(to_f(bcol[(int64_t)q * a.bias_qs]), kLog2e, lterm);
          }
          float p = __builtin_amdgcn_exp2f(fmaf(sacc[i], a.scale_log2, lterm));
          if constexpr (BOUND) {
            const int q = qb + qi;
            const bool valid = (mykey < Sk) && (q < nq) && !(CAUSAL && mykey > q);
            p = valid ? p : 0.f;
          }
          float dpv = dpacc[i];
          float pk = p;
          if constexpr (DROPOUT) {
            const int m = __builtin_amdgcn_sbfe((int)mg4[e], r, 1);
            pk = __builtin_bit_cast(float, __builtin_bit_cast(int, p) & m);
            dpv = __builtin_bit_cast(float, __builtin_bit_cast(int, dpv) & m);
          }
          pd[i] = pk;
          ds[i] = p * fmaf(dpv, rkeep, -dg4[e]);
        }
      }
    };
    if (interior)
      elementwise(std::false_type{});
    else
      elementwise(std::true_type{});
    if constexpr (BIAS) {
      // trainable bias: its gradient is dS (natural domain, before the softmax scale). Lanes of a
      // half hold 32 consecutive keys of one query row per element: coalesced 128-B runs.
      if (a.dbias && mykey < a.Sk) {
        float* dcol = a.dbias + b * a.dbias_bs + h * a.dbias_hs + mykey;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int q = qb + kappa(i, hl);
          if (q < nq) {
            float* dst = dcol + (int64_t)q * a.dbias_qs;
            if (a.dbias_atomic) atomicAdd(dst, ds[i]);
            else *dst = ds[i];
          }
        }
      }
    }
    // dV += P^T . dO : accumulator-as-A (contraction over q = rows), B = dO via tr reads
    // dK += dS^T . Q : same with Q
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const V8 pa = pack8<T, V8>(pd + 8 * s2);
      const V8 sa = pack8<T, V8>(ds + 8 * s2);
      const int kq = 16 * s2 + 4 * hl + ((lane & 15) >> 2);
#pragma unroll
      for (int db = 0; db < D / 32; ++db) {
        const int c0 = 32 * db + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
        const V8 dob = tr_frag<V8>(lds_do, kq, LDQ, c0);
        const V8 qbf = tr_frag<V8>(lds_q, kq, LDQ, c0);
        dv[db] = M::mma(pa, dob, dv[db]);
        dk[db] = M::mma(sa, qbf, dk[db]);
      }
    }
    if constexpr (DQ) {
      // dS^T to LDS as [key][q] (16-bit) for dQ = dS . K
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        typedef T t4 __attribute__((ext_vector_type(4)));
        t4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = (T)ds[4 * g4 + e];  // queries 8 g4 + 4 hl + e
        *(t4*)(lds_ds + dso(32 * wid + r, 8 * g4 + 4 * hl)) = w;
      }
      lds_barrier();
      // dQ^T [D x 32 q] = K^T . dS^T on 16x16x32 MFMAs over the full 128-key contraction: wave
      // w owns query tile qt = w & 1 (16 queries) and D/32 dim tiles of 16 from (w >> 1) D/32;
      // A = K^T rows, B = dS rows (16-byte LDS reads); each lane ends with 4 consecutive dims of
      // one query (8-byte stores). No cross-wave reduction, no scattered 2-byte stores.
      constexpr int NT = D / 32;
      const int qt = wid & 1, dt0 = (wid >> 1) * NT;
      const int lq = lane & 15, lg = lane >> 4;
      f32x4 acc[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < kBwdBK; kk += 32) {
        // B = dS [8 keys x 16 queries]: two transposed 4-key blocks of dS^T (lane 4q'+p of the
        // group addresses key row kk + 8 lg + q', queries 16 qt + 4p; lane lq receives query 16 qt + lq)
        const int dr = kk + 8 * lg + ((lane & 15) >> 2), dc = 16 * qt + 4 * (lane & 3);
        const V8 bb = join4<V8>(lds_tr16(lds_ds + dso(dr, dc)), lds_tr16(lds_ds + dso(dr + 4, dc)));
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const V8 aa = *(const V8*)(lds_k + ((dt0 + t) * 16 + lq) * KT_LD + kk + 8 * lg);
          acc[t] = Mfma16T<T>::mma(aa, bb, acc[t]);
        }
      }
      // this workgroup is the sole writer of these query rows (single key block): final dtype
      const int q = qb + 16 * qt + lq;
      typedef T t4 __attribute__((ext_vector_type(4)));
      uint2 wq[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        t4 w;
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = stored_product<T, DSUM>(acc[t][i], a.scale);
        wq[t] = __builtin_bit_cast(uint2, w);
      }
      // 16-byte stores (as the forward's O, T21): lanes of 16-lane rows lg and lg + 1 hold 4 dims each
      // of the same query for dim tiles t and t + 1; one v_permlane16_swap per dword gives the even
      // rows dims 4 lg .. 4 lg + 7 of tile t and the odd rows those of tile t + 1 (every lane, ahead
      // of the row-validity branch)
      constexpr bool WIDE = NT % 2 == 0;
      uint4 wd[WIDE ? NT / 2 : 1];
      if constexpr (WIDE) {
#pragma unroll
        for (int t = 0; t < NT; t += 2) {
          const auto rx = __builtin_amdgcn_permlane16_swap(wq[t].x, wq[t + 1].x, false, false);
          const auto ry = __builtin_amdgcn_permlane16_swap(wq[t].y, wq[t + 1].y, false, false);
          wd[t / 2] = make_uint4(rx[0], ry[0], rx[1], ry[1]);
        }
      }
      if (q < nq) {
        const int64_t qoff = b * a.dq_bs + h * a.dq_hs + (int64_t)q * a.dq_ss;
        T* dqp = (T*)a.dq + qoff;
        if constexpr (WIDE) {
          if (!a.q8only) {
#pragma unroll
            for (int t = 0; t < NT; t += 2)
              *(uint4*)(dqp + (dt0 + t + (lg & 1)) * 16 + 8 * (lg >> 1)) = wd[t / 2];
          }
        }
        if (a.q8dq) {  // fp8 codes of dq as stored (the QKV input-gradient GEMM's operand)
          uint32_t cq[NT];
#pragma unroll
          for (int t = 0; t < NT; ++t)
            cq[t] = a.q8_fmt == 0 ? f8_codes4<0, T>(wq[t].x, wq[t].y, q8s, q8mx) : f8_codes4<1, T>(wq[t].x, wq[t].y, q8s, q8mx);
          if constexpr (WIDE) {  // the same regrouping: 8-byte stores (rows lg, lg + 1 share the query)
#pragma unroll
            for (int t = 0; t < NT; t += 2) {
              const auto rc = __builtin_amdgcn_permlane16_swap(cq[t], cq[t + 1], false, false);
              *(uint2*)(a.q8dq + qoff + (dt0 + t + (lg & 1)) * 16 + 8 * (lg >> 1)) = make_uint2(rc[0], rc[1]);
            }
          } else {
#pragma unroll
            for (int t = 0; t < NT; ++t) *(uint32_t*)(a.q8dq + qoff + (dt0 + t) * 16 + 4 * lg) = cq[t];
          }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if constexpr (!WIDE) {
            if (!a.q8only) *(uint2*)(dqp + (dt0 + t) * 16 + 4 * lg) = wq[t];
          }
          if constexpr (DSUM) {
            const t4 w = __builtin_bit_cast(t4, wq[t]);
#pragma unroll
            for (int i = 0; i < 4; ++i) dqcs[t][i] += (float)w[i];
          }
        }
      }
    }  // DQ
  };
  if constexpr (DEPTH2) {
    for (int qb = qstart; qb < nq; qb += 2 * kBwdBQ) {
      body(pfa, qb);
      if (qb + kBwdBQ < nq) body(pfb, qb + kBwdBQ);
    }
  } else {
    for (int qb = qstart; qb < nq; qb += kBwdBQ) body(pfa, qb);
  }
  // write dK, dV: element i of block db -> key = k0 + 32 wid + kappa(i, hl), dim = 32 db + r
  T* dkp = (T*)dk_out + b * a.dk_bs + h * a.dk_hs;
  T* dvp = (T*)dv_out + b * a.dv_bs + h * a.dv_hs;
  // optional bias-gradient partials: column sums of the stored dq / dk / dv over positions
  float* dsum = DSUM ? a.dsum + ((int64_t)b * 3 * a.H + h) * D : nullptr;
  if (DSUM && DQ) {  // reduce over the 16 query lanes; both query-tile waves add their partials
    const int lq = lane & 15, lg = lane >> 4, dt0 = (wid >> 1) * (D / 32);
#pragma unroll
    for (int t = 0; t < D / 32; ++t) {
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = dqcs[t][i];
        v[i] = group_sum<16>(v[i]);  // all 16 lanes hold the sum
      }
      // lane lq < 4 of each group adds dim 4 lg + lq: one atomic instruction (16 lanes) per tile
      // (atomics cost per instruction, so 4 single-lane instructions would cost 4x)
      const float x = lq == 0 ? v[0] : lq == 1 ? v[1] : lq == 2 ? v[2] : v[3];
      if (lq < 4) atomicAdd(dsum + (dt0 + t) * 16 + 4 * lg + lq, x);
    }
  }
  // dK then dV staged through LDS so the global stores are 16-byte row chunks. The staging image is
  // [D][keys] (row stride 132 elements = 66 dwords: the 16 rows of a lane group's ds_write_b64 land
  // on distinct bank pairs): each lane writes 4 consecutive keys of one dim per 8-byte store (8 per
  // tensor instead of the 32 ds_write_b16 a [key][D] image takes), and the store loop reads
  // 8 dims of one key with two ds_read_b64_tr_b16 (every lane active: the tr read gathers across
  // lanes).
  lds_barrier();  // every wave is done reading lds_k (dQ products)
  constexpr int LDE = kBwdBK + 4;
  static_assert(D * LDE <= LDSK, "dK/dV staging fits lds_k");
  // DSUM: the four waves' column sums (32 keys each) meet in LDS and are added in wave order, so
  // the bias gradient does not depend on which wave's atomic lands first (four float atomics on one
  // slot rounded differently from run to run). lds_q is free here: its last reads (the final query
  // block's products) are behind the barrier above. One [waves][D] image per emit call.
  static_assert(2 * kBwdWaves * D * sizeof(float) <= kBwdBQ * LDQ * sizeof(T), "column-sum staging fits lds_q");
  auto emit = [&](const f32x16 (&acc)[D / 32], const float mul, T* dst, const int64_t ss, float* dsum_t,
                  uint8_t* q8dst, float* fsum) {
    typedef T t4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int db = 0; db < D / 32; ++db) {
      float sum = 0.f;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int kl0 = 32 * wid + 8 * g4 + 4 * hl;  // keys kl0 .. kl0 + 3
        t4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          w[e] = stored_product<T, DSUM>(acc[db][4 * g4 + e], mul);
          if constexpr (DSUM) sum += (k0 + kl0 + e < a.Sk) ? (float)w[e] : 0.f;
        }
        *(t4*)(lds_k + (32 * db + r) * LDE + kl0) = w;
      }
      if constexpr (DSUM) {
        sum += xor32_f(sum);
        if (hl == 0) fsum[wid * D + 32 * db + r] = sum;
      }
    }
    lds_barrier();
    if constexpr (DSUM) {
      // one contribution per workgroup and slot (several key blocks of one head still meet here)
      if (threadIdx.x < D) {
        const float* f = fsum + threadIdx.x;
        static_assert(kBwdWaves == 4, "fixed-order sum over the four waves");
        atomicAdd(dsum_t + threadIdx.x, ((f[0] + f[D]) + f[2 * D]) + f[3 * D]);
      }
    }
    // 16-lane group tasks: (8-dim block, 16-key block); a wave's 4 groups take 4 consecutive dim
    // blocks of the same keys (64 contiguous bytes of each key row per store instruction)
    constexpr int NDB = D / 8, NTASK = NDB * (kBwdBK / 16);
    static_assert(NTASK % 16 == 0, "tasks per workgroup");
    // fp8 codes of the stored values (the same element offset in the code array), 16 bytes per
    // lane: the 16-lane groups g (even) and g + 1 hold adjacent 8-dim blocks of the same keys, so
    // for iterations it and it + 1 one v_permlane16_swap per dword gives the even groups 16 dims of
    // their iteration-it key and the odd groups 16 dims of their iteration-(it + 1) key — half the
    // code store instructions
    constexpr bool CPAIR = (NTASK / 16) % 2 == 0 && NDB % 2 == 0;
    uint2 cprev = make_uint2(0u, 0u);
    int kprev = 0, dprev = 0;
#pragma unroll
    for (int it = 0; it < NTASK / 16; ++it) {
      const int t = it * 16 + wid * 4 + (lane >> 4);
      const int d0 = (t % NDB) * 8, kb = (t / NDB) * 16;
      const T* src = lds_k + (d0 + ((lane & 15) >> 2)) * LDE + kb + 4 * (lane & 3);
      const s16x4 lo = lds_tr16(src), hi = lds_tr16(src + 4 * LDE);
      const int key = k0 + kb + (lane & 15);
      const V8 x = join4<V8>(lo, hi);
      if (key < a.Sk && !a.q8only) *(V8*)(dst + (int64_t)key * ss + d0) = x;
      if (q8dst) {
        const uint4 ww = __builtin_bit_cast(uint4, x);
        uint2 c;
        float mx = 0.f;  // only keys in range feed the amax
        if (a.q8_fmt == 0) {
          c.x = f8_codes4<0, T>(ww.x, ww.y, q8s, mx);
          c.y = f8_codes4<0, T>(ww.z, ww.w, q8s, mx);
        } else {
          c.x = f8_codes4<1, T>(ww.x, ww.y, q8s, mx);
          c.y = f8_codes4<1, T>(ww.z, ww.w, q8s, mx);
        }
        if (key < a.Sk) q8mx = fmaxf(q8mx, mx);
        if constexpr (CPAIR) {
          if (it & 1) {  // every lane swaps (outside the key branch)
            const auto sx = __builtin_amdgcn_permlane16_swap(cprev.x, c.x, false, false);
            const auto sy = __builtin_amdgcn_permlane16_swap(cprev.y, c.y, false, false);
            const bool odd = (lane >> 4) & 1;
            const int kk = odd ? key : kprev, dd = odd ? d0 - 8 : dprev;
            if (kk < a.Sk) *(uint4*)(q8dst + (int64_t)kk * ss + dd) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
          } else {
            cprev = c;
            kprev = key;
            dprev = d0;
          }
        } else if (key < a.Sk) {
          *(uint2*)(q8dst + (int64_t)key * ss + d0) = c;
        }
      }
    }
    lds_barrier();
  };
  emit(dk, a.scale, dkp, a.dk_ss, DSUM ? dsum + (int64_t)a.H * D : nullptr,
       a.q8dk ? a.q8dk + b * a.dk_bs + h * a.dk_hs : nullptr, (float*)lds_q);
  emit(dv, rkeep, dvp, a.dv_ss, DSUM ? dsum + (int64_t)2 * a.H * D : nullptr,
       a.q8dv ? a.q8dv + b * a.dv_bs + h * a.dv_hs : nullptr, (float*)lds_q + kBwdWaves * D);
  if (a.q8dq) f8_block_amax(q8mx, a.q8_amax, q8seen);  // every thread of the block reaches this
}

// dQ for key ranges longer than one backward key block: query-stationary, the forward's
// structure (one workgroup = 4 waves x 32 query rows, K/V streamed in 64-key tiles):
//   S^T = K . Q^T and dP^T = V . dO^T (32x32x16, one query per lane, so lse and delta are
//   lane-local scalars), dS^T = P^T * (dP^T * keep - delta) in registers, and
//   dQ^T += K^T . dS^T with the dS^T accumulators reused directly as the B operand (the same
//   register reuse as O^T += V^T . P^T in the forward). Every dQ row has exactly one writer:
//   no fp32 atomics, no accumulator buffer, no conversion pass. The extra S / dP products (vs
//   the fused single-kernel backward) cost less than the fp32 atomic traffic they replace.
template <typename T, int D, bool CAUSAL, bool DROPOUT, bool DSUM, bool BIAS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D <= 64 ? 2 : 1, D <= 64 ? 2 : 1))) attn_bwd_dq_kernel(AttnArgs a, const void* dout, const float* delta_in) {
  using M = MfmaT<T>;
  using V8 = typename M::V8;
  constexpr int LDR = ld_rows<D>();  // V: row reads
  constexpr int LDK = ld_both<D>();  // K: row and transposed reads
  __shared__ __attribute__((aligned(16))) T lds_k[kFwdKB * LDK];
  __shared__ __attribute__((aligned(16))) T lds_v[kFwdKB * LDR];

  // wid through readfirstlane: wave-uniform in SGPRs, so tile-level conditions become scalar branches
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, hl = lane >> 5;
  const int bh = blockIdx.x;  // grid (B*H, query blocks), heaviest (causal: last) query blocks first
  const int b = bh / a.H, h = bh % a.H;
  const int q0 = (CAUSAL ? gridDim.y - 1 - blockIdx.y : blockIdx.y) * kFwdBQ;
  const int qrow = q0 + 32 * wid + r;
  const int Sk = a.k_lens ? min(a.k_lens[b], a.Sk) : a.Sk;

  const T* qp = (const T*)a.q + b * a.q_bs + h * a.q_hs;
  const T* dop = (const T*)dout + b * a.do_bs + h * a.do_hs;
  const int hk = kv_head(a, h);
  const T* kp = (const T*)a.k + b * a.k_bs + hk * a.k_hs;
  const T* vp = (const T*)a.v + b * a.v_bs + hk * a.v_hs;
  const T* brow = BIAS ? bias_row<T>(a, b, h, qrow) : nullptr;

  // Q^T and dO^T fragments (B operands): lane (q=r, hl) holds X[q][16s + 8hl .. +7]
  V8 qf[D / 16], df[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    if (qrow < a.Sq) {
      qf[s] = *(const V8*)(qp + (int64_t)qrow * a.q_ss + 16 * s + 8 * hl);
      df[s] = *(const V8*)(dop + (int64_t)qrow * a.do_ss + 16 * s + 8 * hl);
    } else {
      qf[s] = V8{};
      df[s] = V8{};
    }
  }
  // log2-domain lse (+inf for padding rows and fully masked rows: P = 0) and delta
  const float lse2 = qrow < a.Sq ? a.lse[(int64_t)bh * a.Sq + qrow] * kLog2e : INFINITY;
  const float delta = qrow < a.Sq ? delta_in[(int64_t)bh * a.Sq + qrow] : 0.f;

  f32x16 dq[D / 32];
#pragma unroll
  for (int i = 0; i < D / 32; ++i) dq[i] = f32x16{};

  int kend = Sk;
  if (CAUSAL) kend = min(kend, q0 + kFwdBQ);
  const int ntiles = (kend + kFwdKB - 1) / kFwdKB;

  constexpr int CPR = D / 8;
  constexpr int CH = kFwdKB * CPR / 256;
  // K/V tiles of the tile TWO ahead are loaded into registers while the current tile computes
  // (two register sets, loop unrolled by two) at D <= 64; one ahead at D >= 128 (register budget)
  constexpr bool KV2 = D <= 64;
  constexpr int AHEAD = KV2 ? 2 : 1;
  struct KV {
    uint4 k[CH], v[CH];
    uint32_t m[2];
  };
  KV kva, kvb;
  const uint32_t* mrow =
      DROPOUT && qrow < a.Sq ? (const uint32_t*)(a.dmask + ((int64_t)bh * a.Sq + qrow) * a.mask_words) : nullptr;
  // (gload / lstore are attn_fwd_kernel's written out again: shared, they change the assembly)
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
    if (DROPOUT) {
      // the forward's keep bits for this lane's 16 keys of each 32-key block (same layout)
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
        const int blk = (kt * kFwdKB >> 5) + sb;
        R.m[sb] = 0u;
        if (mrow && blk * 32 < a.Sk) R.m[sb] = mrow[blk];  // raw: shifted at use (no wait here)
      }
    }
  };
  auto lstore = [&](KV& R) {
    uint4 (&kreg)[CH] = R.k;
    uint4 (&vreg)[CH] = R.v;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int idx = threadIdx.x + 256 * c;
      const int row = idx / CPR, col = (idx % CPR) * 8;
      *(uint4*)(lds_k + row * LDK + col) = kreg[c];
      *(uint4*)(lds_v + row * LDR + col) = vreg[c];
    }
  };

  const float rkeep = a.drop_scale;
  if (ntiles > 0) gload(kva, 0);
  if (KV2 && ntiles > 1) gload(kvb, 1);
  auto tile = [&](KV& R, const int kt) {
    if constexpr (D >= 128) {
      // pin the dQ accumulators to AGPRs at the tile boundary: without it the allocator copied all
      // 64 of them to VGPRs and back every tile so the S / dP products could use their AGPRs
#pragma unroll
      for (int i = 0; i < D / 32; ++i) asm volatile("" : "+a"(dq[i]));
    }
    lds_barrier();  // previous tile fully consumed
    lstore(R);
    const uint32_t mcur[2] = {R.m[0] >> (4 * hl), R.m[1] >> (4 * hl)};
    lds_barrier();
    if (kt + AHEAD < ntiles) gload(R, kt + AHEAD);
    const int kb = kt * kFwdKB;

    f32x16 st[2], dpt[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      V8 kf[D / 16], vf[D / 16];
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        kf[s] = *(const V8*)(lds_k + (32 * sb + r) * LDK + 16 * s + 8 * hl);
        vf[s] = *(const V8*)(lds_v + (32 * sb + r) * LDR + 16 * s + 8 * hl);
      }
      __builtin_amdgcn_sched_group_barrier(0x100, 2 * (D / 16), 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * (D / 16), 0);
      st[sb] = f32x16{};
      dpt[sb] = f32x16{};
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        st[sb] = M::mma(kf[s], qf[s], st[sb]);
        dpt[sb] = M::mma(vf[s], df[s], dpt[sb]);
      }
    }
    const bool interior = (kb + kFwdKB <= Sk) && (!CAUSAL || kb + kFwdKB - 1 <= q0 + 32 * wid);
    const int lim = CAUSAL ? min(Sk, qrow + 1) : Sk;
    float bl2[2][16];  // BIAS: bias x log2(e) of element (sb, i)
    if constexpr (BIAS) {
#pragma unroll
      for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float bv[4];
          bias4<T>(brow, kb + 32 * sb + 8 * g + 4 * hl, a.Sk, bv);
#pragma unroll
          for (int e = 0; e < 4; ++e) bl2[sb][4 * g + e] = bv[e] * kLog2e;
        }
    }
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float p = __builtin_amdgcn_exp2f(fmaf(st[sb][i], a.scale_log2, BIAS ? bl2[sb][i] - lse2 : -lse2));
        if (!interior) {
          if (kb + 32 * sb + kappa(i, hl) >= lim) p = 0.f;
        }
        float dp = dpt[sb][i];
        if (DROPOUT)  // mcur is shifted by 4 hl: bit kappa(i) is this lane's key
          dp = __builtin_bit_cast(float, __builtin_bit_cast(int, dp) & __builtin_amdgcn_sbfe((int)mcur[sb], kappa(i), 1));
        st[sb][i] = p * fmaf(dp, rkeep, -delta);  // dS^T (the softmax scale is applied once, at the end)
      }
    }
    // dQ^T += K^T . dS^T
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float sv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) sv[j] = st[sb][8 * s2 + j];
        const V8 sf = pack8<T, V8>(sv);
        const int k0 = 32 * sb + 16 * s2 + 4 * hl + ((lane & 15) >> 2);
#pragma unroll
        for (int db = 0; db < D / 32; ++db) {
          const int c0 = 32 * db + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
          dq[db] = M::mma(tr_frag<V8>(lds_k, k0, LDK, c0), sf, dq[db]);
        }
      }
    }
  };
  if constexpr (KV2) {
    for (int kt = 0; kt < ntiles; kt += 2) {
      tile(kva, kt);
      if (kt + 1 < ntiles) tile(kvb, kt + 1);
    }
  } else {
    for (int kt = 0; kt < ntiles; ++kt) tile(kva, kt);
  }
  // ---- epilogue: element 4g+e of block db -> dim 32db + 8g + 4hl + e of query qrow; 16-byte
  // stores through one v_permlane32_swap per dword and column-group pair (as the forward's O)
  float* dsum = DSUM ? a.dsum + ((int64_t)b * 3 * a.H + h) * D : nullptr;
  T* dqrow = (T*)a.dq + b * a.dq_bs + h * a.dq_hs + (int64_t)qrow * a.dq_ss;
#pragma unroll
  for (int db = 0; db < D / 32; ++db) {
    typedef T t4 __attribute__((ext_vector_type(4)));
    uint2 wv[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      t4 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = stored_product<T, DSUM>(dq[db][4 * g + e], a.scale);
      wv[g] = __builtin_bit_cast(uint2, w);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const auto rx = __builtin_amdgcn_permlane32_swap(wv[2 * j].x, wv[2 * j + 1].x, false, false);
      const auto ry = __builtin_amdgcn_permlane32_swap(wv[2 * j].y, wv[2 * j + 1].y, false, false);
      if (qrow < a.Sq) *(uint4*)(dqrow + 32 * db + 16 * j + 8 * hl) = make_uint4(rx[0], ry[0], rx[1], ry[1]);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const t4 w = __builtin_bit_cast(t4, wv[g]);
      if constexpr (DSUM) {
        // column sums of the stored values over this wave's 32 query rows (lanes r), then one
        // atomic per dim per wave
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float t = qrow < a.Sq ? (float)w[e] : 0.f;
          t = group_sum<32>(t);
          if (r == 0) atomicAdd(dsum + 32 * db + 8 * g + 4 * hl + e, t);
        }
      }
    }
  }
}

}  // namespace apex
