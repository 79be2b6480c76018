// MFMA GEMM (gemm.hip), device side 2 of 3: the epilogue classes, the GELU math and the fused
// epilogue shared by both kernels (the epilogues are listed at the top of gemm.hip).
#pragma once
#include "gemm_mainloop.h"
#include "fp8_pack.h"

namespace apex {
namespace {

// What an epilogue (GemmEpi) does, by class: the kernels, the persistent kernel's store count
// (epi_stores) and the fp8 launcher all decide from these
constexpr bool epi_gelu_d(int e) { return e == EPI_BIAS_GELU_D || e == EPI_BIAS_GELU_TANH_D; }  // stores gelu'(H)
constexpr bool epi_gelu_fwd(int e) { return e == EPI_BIAS_GELU || e == EPI_BIAS_GELU_TANH || epi_gelu_d(e); }
constexpr bool epi_dgelu(int e) { return e == EPI_DGELU || e == EPI_DGELU_TANH; }
constexpr bool epi_tanh(int e) { return e == EPI_BIAS_GELU_TANH || e == EPI_DGELU_TANH || e == EPI_BIAS_GELU_TANH_D; }
constexpr bool epi_colsum(int e) { return epi_dgelu(e) || e == EPI_MUL; }              // bias-gradient partials
constexpr bool epi_aux_in(int e) { return epi_colsum(e) || e == EPI_RESID; }           // reads an [M, N] input
constexpr bool epi_has_bias(int e) { return e == EPI_BIAS || epi_gelu_fwd(e); }
// fp8 GEMMs: the epilogues that can also write C's fp8 codes (the MLP's hidden activation forward, its
// gradient backward), and of those the ones that can write the codes alone (Q8Out::only)
constexpr bool epi_codes_ok(int e) { return epi_gelu_fwd(e) || epi_colsum(e); }
constexpr bool epi_codes_only_ok(int e) { return epi_gelu_d(e) || e == EPI_MUL; }

// Epilogue switches (template argument XD): bits 0 and 1 are lab diagnostics (tools/gemmlab LAB_PXD,
// production 0), bit 4 is the production codes-only output
constexpr int kEpiNoMath = 1;      // the stored values are the rounded accumulators; same loads and stores
constexpr int kEpiNoStore = 2;     // no global store
constexpr int kEpiCodesOnly = 16;  // C itself is not stored, its fp8 codes are (see epilogue())

// Branch-free erf (Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7): one v_rcp, one v_exp and
// seven FMAs instead of ocml's erff (whose inlined branches made the epilogue 10x larger).
// Two values at a time: the polynomial runs on packed f32 (v_pk_fma_f32 / v_pk_mul_f32), the
// epilogue is VALU-bound on the GELU work (it runs after the MFMA main loop, not beside it).
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 splat(float v) { return f32x2{v, v}; }

// Phi(x) = 0.5 (1 + erf(x / sqrt 2)) given e = exp(-x^2 / 2), the same A&S 7.1.26 polynomial with
// the 1/sqrt(2) folded into p and the 0.5 into the coefficients: Phi = 0.5 + sign(x) (0.5 - q),
// q = poly'(t) t e (two packed instructions fewer per pair than
// evaluating erf(x / sqrt 2) and then 0.5 (1 + erf))
__device__ __forceinline__ f32x2 cdf2(f32x2 x, f32x2 e) {
  const f32x2 ax = __builtin_elementwise_abs(x);
  const f32x2 d = pk_fma(splat(0.3275911f * 0.70710678118654752f), ax, splat(1.f));
  const f32x2 t = f32x2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
  f32x2 p = pk_fma(splat(0.5f * 1.061405429f), t, splat(0.5f * -1.453152027f));
  p = pk_fma(p, t, splat(0.5f * 1.421413741f));
  p = pk_fma(p, t, splat(0.5f * -0.284496736f));
  p = pk_fma(p, t, splat(0.5f * 0.254829592f));
  const f32x2 r = pk_fma(-p * t, e, splat(0.5f));  // 0.5 erf(|x| / sqrt 2)
  return splat(0.5f) + f32x2{copysignf(r[0], x[0]), copysignf(r[1], x[1])};
}
// exp(-x^2/2) via v_exp_f32 (2^y)
__device__ __forceinline__ f32x2 exp_neg_half_sq2(f32x2 x) {
  const f32x2 y = splat(-0.72134752044448170f) * x * x;
  return f32x2{__builtin_amdgcn_exp2f(y[0]), __builtin_amdgcn_exp2f(y[1])};
}
__device__ __forceinline__ f32x2 gelu2(f32x2 x) { return x * cdf2(x, exp_neg_half_sq2(x)); }
// tanh-approximated GELU (GPT-2): x * sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3)
__device__ __forceinline__ f32x2 sig2u(f32x2 x) {
  const f32x2 u = splat(-2.f * 0.7978845608028654f * 1.4426950408889634f) * pk_fma(splat(0.044715f) * x, x * x, x);
  const f32x2 d = splat(1.f) + f32x2{__builtin_amdgcn_exp2f(u[0]), __builtin_amdgcn_exp2f(u[1])};
  return f32x2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
}
__device__ __forceinline__ f32x2 gelu_tanh2(f32x2 x) { return x * sig2u(x); }
__device__ __forceinline__ f32x2 gelu_tanh_grad2(f32x2 x) {
  const f32x2 sg = sig2u(x);
  const f32x2 du = splat(2.f * 0.7978845608028654f) * pk_fma(splat(3.f * 0.044715f) * x, x, splat(1.f));
  return pk_fma(x * sg * (splat(1.f) - sg), du, sg);
}
// gelu(x) and gelu'(x) from one exp / erf (or one sigmoid for the tanh form)
__device__ __forceinline__ void gelu_and_grad2(f32x2 x, bool tanh_form, f32x2& y, f32x2& g) {
  if (tanh_form) {
    const f32x2 sg = sig2u(x);
    y = x * sg;
    const f32x2 du = splat(2.f * 0.7978845608028654f) * pk_fma(splat(3.f * 0.044715f) * x, x, splat(1.f));
    g = pk_fma(y * (splat(1.f) - sg), du, sg);
  } else {
    const f32x2 e = exp_neg_half_sq2(x);
    const f32x2 cdf = cdf2(x, e);
    y = x * cdf;
    g = pk_fma(x * splat(0.39894228040143268f), e, cdf);
  }
}
__device__ __forceinline__ f32x2 gelu_grad2(f32x2 x) {
  const f32x2 e = exp_neg_half_sq2(x);
  const f32x2 cdf = cdf2(x, e);
  return pk_fma(x * splat(0.39894228040143268f), e, cdf);
}

template <typename T>
__device__ __forceinline__ void load4(const T* p, float (&v)[4]) {
  Pack<T, 4> pk = *reinterpret_cast<const Pack<T, 4>*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = to_f(pk.v[i]);
}
template <typename T>
__device__ __forceinline__ void store4(T* p, const float (&v)[4]) {
  Pack<T, 4> pk;
#pragma unroll
  for (int i = 0; i < 4; ++i) pk.v[i] = from_f<T>(v[i]);
  *reinterpret_cast<Pack<T, 4>*>(p) = pk;
}

// Buffer resource for a wave-uniform base address (the epilogue's full-tile path): every lane
// addresses rows through ONE 32-bit voffset plus an SGPR soffset per row slot, instead of a 64-bit
// VGPR address pair per access (32 pairs per lane for a load+store epilogue, which the scheduler
// hoisted and spilled). Inputs go through readfirstlane so no waterfall loop is emitted
// (cdna_hip_programming.md T8 / T20).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wave_rsrc(const void* p, uint32_t bytes) {
  const uint64_t a = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), (short)0,
                                           (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

// Epilogue shared by both kernels (wave tile 128 x 64 at rows m0 + wr*128, cols n0 + wc*64).
// Rounds the accumulators of a 128 x 64 wave tile (acc[J0 .. J0+3][*]) to T and writes them into the
// wave's 16 KB LDS region in the layout the epilogue reads back (see epilogue()).
// I0 / NI: the fragment rows staged (NI = 4: one 64-row half of the wave tile into an 8 KB region,
// local rows 0..63; the row's XOR pattern only depends on row & 15, so it is the same either way)
template <typename T, int J0, int NJ, int I0 = 0, int NI = 8>
__device__ __forceinline__ void stage_acc(const f32x4 (&acc)[NJ][8], char* reg, int lane, float alpha) {
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int ii = 0; ii < NI; ++ii) {
      const int i = I0 + ii;
      const int row = ii * 16 + lr;
      const int chunk = (2 * j + (lk >> 1)) ^ (row & 7);
      const int half = (lk & 1) ^ ((row >> 3) & 1);
      Pack<T, 4> pk;
#pragma unroll
      for (int e = 0; e < 4; ++e) pk.v[e] = from_f<T>(acc[J0 + j][i][e] * alpha);
      *reinterpret_cast<Pack<T, 4>*>(reg + row * 128 + chunk * 16 + half * 8) = pk;
    }
}

// STAGED: the accumulators are already in `reg` (stage_acc), `acc` is not read
// Q8 (1 + fp8 format, 0 = off): the C output's fp8 codes are written too (q8.y, ldc bytes per row,
// scaled by q8.scale[0], max|C| into q8.amax) — the next GEMM's fp8 operand without a standalone
// quantise pass over C
// Loads the compiler does not see (the persistent kernel's epilogue): with LDS-DMA pieces of the next
// tile in flight, hipcc waits vmcnt(0) before the first use of any load it issued itself, i.e. the
// epilogue would stall on the next tile's prologue. These load through a descriptor held in SGPRs
// (built from wave-uniform values: s_nop 4 covers the SGPR-write -> buffer-read hazard) and are
// retired by explicit counted waits (asm_wait8 / asm_wait16) that name every destination register.
typedef unsigned u32x4g __attribute__((ext_vector_type(4)));
typedef int i32x4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4s sgpr_rsrc(const void* p, uint32_t bytes) {
  const uint64_t a = (uint64_t)p;
  return i32x4s{(int)__builtin_amdgcn_readfirstlane((uint32_t)a),
                (int)__builtin_amdgcn_readfirstlane((uint32_t)(a >> 32)) & 0xffff,
                (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000};
}
__device__ __forceinline__ u32x4g asm_load16(const i32x4s& rs, uint32_t voff, int soff) {
  u32x4g d;
  asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(d) : "v"(voff), "s"(rs), "s"(soff) : "memory");
  return d;
}
template <int N>
__device__ __forceinline__ void asm_wait(u32x4g (&r)[8]) {
  asm volatile("s_waitcnt vmcnt(%8)"
               : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7])
               : "n"(N)
               : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <int N>
__device__ __forceinline__ void asm_wait1(u32x4g& r) {
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(r) : "n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
struct NoHook {
  __device__ __forceinline__ void operator()() const {}
};

// HALVES (the persistent kernel): `reg` is an 8 KB region; each 64-row half of the wave tile is staged
// into it right before its 8 row slots are read back (the other 64 KB of LDS hold the next tile's
// first K-tile meanwhile)
// With HALVES the epilogue's own loads (bias, [M, N] input) are asm loads issued BEFORE `pre()` (the
// caller's hook: the next tile's LDS-DMA pieces, exactly 8 per wave) and retired by counted waits that
// leave those pieces (and this epilogue's stores) in flight.
// XD: kEpiNoMath / kEpiNoStore (lab diagnostics) and kEpiCodesOnly (production, fp8 codes-only outputs,
// Q8Out::only): C itself is not stored — its fp8 codes (and the GELU_D derivative / the MUL bias-grad
// partials) are: the fp8 step's consumers of the MLP hidden activation and its gradient read only the
// codes (apex.fp8 codes_only_ok)
template <typename T, int EPI, bool EDGE, int J0 = 0, int NJ = 4, bool STAGED = false, int Q8 = 0,
          bool HALVES = false, typename Hook = NoHook, int XD = 0>
__device__ __forceinline__ void epilogue(const f32x4 (&acc)[NJ][8], char* reg, T* __restrict__ C, int M, int N,
                                         int64_t ldc, const T* __restrict__ bias, const T* __restrict__ aux,
                                         int64_t ldaux, T* __restrict__ aux_out, float* __restrict__ part, int m0,
                                         int n0, int tm, int wr, int wc, int lane, float alpha = 1.f,
                                         const Q8Out& q8 = Q8Out{}, const Hook& pre = Hook{},
                                         float* q8_defer = nullptr) {
  // HALVES + Q8: the codes of the multiply / dGELU epilogues are stashed and emitted per half, and the
  // running max|C| goes to *q8_defer (the persistent kernel issues one amax atomic per workgroup at its
  // end: an atomic here would sit between the next tile's LDS-DMA pieces and their counted wait)
  static_assert(!HALVES || (!STAGED && !EDGE), "halved staging: full tiles, accumulators in registers");
  const int lr = lane & 15, lk = lane >> 4;
  // acc[j][i] holds rows wr*128 + i*16 + lr, cols wc*64 + j*16 + 4*lk .. +3 of the tile. The fp32
  // accumulators are rounded to T and transposed through the wave's own 16 KB LDS region
  // ([128 rows][64 cols], 16-B chunks XOR-swizzled by row, 8-B halves swapped on rows 8..15 of every
  // 16 so the ds_write_b64 groups are conflict-free); then every lane owns 8 consecutive columns of
  // 16 rows ("row slots" it = 0..15, rows lane/8 + 8 it of the wave tile), and the epilogue math
  // (bias, GELU, dGELU, residual) runs on 16-byte vectors with 16-byte loads/stores (8 lanes = one
  // 128-B row run). Rounding before the bias matches the unfused composition (GEMM output in T,
  // then the bias/activation kernel in fp32).
  //
  // Register budget (the kernel runs at 256 VGPRs): the slots are processed in two halves of 8, and
  // the [M, N] input operand of EPI_RESID / EPI_MUL / EPI_DGELU is loaded a half AHEAD — the first
  // half's 8 x 16 B per lane are issued before the accumulators go through LDS (the HBM latency
  // hides behind the transposition), the second half's while the first half computes and stores.
  // Global accesses go through buffer resources based at the wave tile's origin: full tiles use one
  // per-lane voffset plus an SGPR soffset per slot; edge tiles a per-slot voffset that points past
  // the resource for rows >= M or columns >= N (loads return 0, stores are dropped). With 64-bit
  // flat addresses per access and all 16 slots at once, these epilogues spilled 120-340 B per lane
  // to scratch (137 scratch instructions in EPI_MUL).
  // Measured alternative (profiles/r2_gemm_regroup_epilogue_ab.jsonl): the accumulators regrouped
  // in registers by v_permlane16_swap instead of the LDS transposition (no LDS, no barrier, every
  // lane 8 consecutive columns) — correct, but 2-10 % SLOWER (FFN2 dgrad x gelu' 796 -> 869 us):
  // each 16-byte-per-lane access then covers 16 rows x 64 B instead of 8 rows x 128 B.
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  constexpr bool GELU_D = epi_gelu_d(EPI), GELU_FWD = epi_gelu_fwd(EPI), DGELU = epi_dgelu(EPI), MUL = EPI == EPI_MUL;
  constexpr bool COLSUM = epi_colsum(EPI), TANH = epi_tanh(EPI), AUX_IN = epi_aux_in(EPI), HAS_BIAS = epi_has_bias(EPI);

  const int ncol = n0 + wc * 64 + (lane & 7) * 8;
  const int wrow0 = m0 + wr * 128, wcol0 = n0 + wc * 64;
  const int lrow = lane >> 3, lcol = (lane & 7) * 8;
  auto wave_res = [&](const T* base, int64_t ld) {
    return wave_rsrc(base + (int64_t)wrow0 * ld + wcol0, (uint32_t)(128 * ld * (int64_t)sizeof(T)));
  };
  // bounds-aware per-slot offset (any tile)
  auto voff_g = [&](int64_t ld, int slot) -> uint32_t {
    const int r = lrow + slot * 8;
    return (wrow0 + r < M && ncol < N) ? (uint32_t)((r * ld + lcol) * (int64_t)sizeof(T)) : 0x80000000u;
  };
  const __amdgpu_buffer_rsrc_t rs_c = wave_res(C, ldc);
  __amdgpu_buffer_rsrc_t rs_o = rs_c, rs_x = rs_c, rs_q = rs_c;
  float q8s = 0.f, q8mx = 0.f;
  if constexpr (Q8 != 0) {
    q8s = q8.scale[0];
    rs_q = wave_rsrc(q8.y + (int64_t)wrow0 * ldc + wcol0, (uint32_t)(128 * ldc));
  }
  if constexpr (GELU_FWD) rs_o = wave_res(aux_out, ldc);
  if constexpr (AUX_IN) rs_x = wave_res(aux, ldaux);
  auto unpack = [&](const u32x4& x, float (&v)[8]) {
    Pack<T, 8> pk = *reinterpret_cast<const Pack<T, 8>*>(&x);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = to_f(pk.v[e]);
  };
  auto pack = [&](const float (&v)[8]) {
    Pack<T, 8> pk;
#pragma unroll
    for (int e = 0; e < 8; ++e) pk.v[e] = from_f<T>(v[e]);
    return *reinterpret_cast<const u32x4*>(&pk);
  };

  // F (EDGE = false: the launch has only full tiles, M % 256 == 0 and N % 256 == 0) or the
  // bounds-checked form for every tile. One variant per kernel, no runtime branch: with both
  // variants in one kernel the compiler hoisted their common code (conversions, LDS reads,
  // unpacks) above the branch and spilled.
  {
    constexpr bool F = !EDGE;
    auto voff = [&](int64_t ld, int slot) -> uint32_t {
      if constexpr (F) return (uint32_t)((lrow * ld + lcol) * (int64_t)sizeof(T));
      return voff_g(ld, slot);
    };
    auto soff = [&](int64_t ld, int slot) -> int { return F ? (int)(slot * 8 * ld * (int64_t)sizeof(T)) : 0; };
    // stores take the slot offset in voffset with soffset = 0: with a register soffset hipcc
    // (ROCm 7.2) does not count the gfx950 store-data hazard — a VALU overwrote the data VGPRs of
    // a buffer_store_dwordx4 right after issue and corrupted a dword of the stored row (seen on
    // the GPU: sporadic dwords of EPI_BIAS_GELU's pre-activation output)
    // Measured alternative: non-temporal stores of C and / or the second output — neutral in the step
    // (profiles/README.md, "non-temporal epilogue stores")
    auto st = [&](const __amdgpu_buffer_rsrc_t& rs, int slot, const u32x4& x) {
      if constexpr (XD & kEpiNoStore) {  // keep the value live
        asm volatile("" ::"v"(x));
      } else {
        __builtin_amdgcn_raw_buffer_store_b128(x, rs, voff(ldc, slot) + (uint32_t)soff(ldc, slot), 0, 0);
      }
    };
    // first half of the input operand in flight (sched_barriers pin the phase order: left alone,
    // the scheduler hoists both halves' loads above the transposition and spills around them)
    u32x4 ra[8];
    u32x4g braw = u32x4g{0u, 0u, 0u, 0u};
    i32x4s rsx_s = i32x4s{0, 0, 0, 0};
    if constexpr (HALVES) {
      if constexpr (AUX_IN) {
        rsx_s = sgpr_rsrc(aux + (int64_t)wrow0 * ldaux + wcol0, (uint32_t)(128 * ldaux * (int64_t)sizeof(T)));
#pragma unroll
        for (int it = 0; it < 8; ++it) ra[it] = asm_load16(rsx_s, voff(ldaux, it), soff(ldaux, it));
        pre();
        __builtin_amdgcn_sched_barrier(0);
        stage_acc<T, J0, NJ, 0, 4>(acc, reg, lane, alpha);
        __builtin_amdgcn_sched_barrier(0);
        asm_wait<8>(ra);  // the 8 pieces of pre() are younger
      } else {
        if constexpr (HAS_BIAS) braw = asm_load16(sgpr_rsrc(bias + n0 + wc * 64, 128), (uint32_t)((lane & 7) * 16), 0);
        pre();
        __builtin_amdgcn_sched_barrier(0);
        stage_acc<T, J0, NJ, 0, 4>(acc, reg, lane, alpha);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (HAS_BIAS) asm_wait1<8>(braw);
      }
    } else if constexpr (AUX_IN) {
#pragma unroll
      for (int it = 0; it < 8; ++it) ra[it] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, voff(ldaux, it), soff(ldaux, it), 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!STAGED && !HALVES) stage_acc<T, J0, NJ>(acc, reg, lane, alpha);
    __builtin_amdgcn_sched_barrier(0);
    float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (HAS_BIAS) {
      if constexpr (HALVES) {
        unpack(*reinterpret_cast<const u32x4*>(&braw), bv);
      } else {
        const int nc = ncol < N ? ncol : N - 8;  // (N % 8 == 0: edge lanes read a valid chunk, unused)
        unpack(*reinterpret_cast<const u32x4*>(bias + nc), bv);
      }
    }
    float csum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    u32x4 rb[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      u32x4 rc[8];
      if constexpr (HALVES) {
        if (h == 1) {  // (half 0 was staged before the first wait; LDS ops of one wave run in order)
          stage_acc<T, J0, NJ, 4, 4>(acc, reg, lane, alpha);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int row = ((HALVES ? 0 : 8 * h) + it) * 8 + lrow, c = lane & 7;
        u32x4 x = *reinterpret_cast<const u32x4*>(reg + row * 128 + ((c ^ (row & 7)) << 4));
        if ((row >> 3) & 1) x = u32x4{x[2], x[3], x[0], x[1]};
        rc[it] = x;
      }
      if constexpr (AUX_IN) {
        if constexpr (HALVES) {
          // second half of the input: issued now, retired at h = 1 behind the 8 stores of h = 0
          if (h == 0) {
#pragma unroll
            for (int it = 0; it < 8; ++it) rb[it] = asm_load16(rsx_s, voff(ldaux, 8 + it), soff(ldaux, 8 + it));
          } else {
            asm_wait<Q8 != 0 ? 16 : 8>(rb);  // (half 0's stores, and with Q8 its codes, are younger)
          }
        } else if (h == 0) {
#pragma unroll
          for (int it = 0; it < 8; ++it)
            rb[it] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, voff(ldaux, 8 + it), soff(ldaux, 8 + it), 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int slot = 8 * h + it;
        u32x4 out = rc[it];
        if constexpr ((XD & kEpiNoMath) && EPI != EPI_NONE) {  // same bytes, no math
          if constexpr (GELU_D) st(rs_o, slot, out);
          if constexpr (AUX_IN) out = out ^ (h == 0 ? ra[it] : rb[it]);
        } else if constexpr (EPI != EPI_NONE) {
          float v[8];
          unpack(rc[it], v);
          if constexpr (EPI == EPI_BIAS) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += bv[e];
          } else if constexpr (GELU_FWD) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += bv[e];
            if constexpr (!GELU_D) {
              const u32x4 hraw = pack(v);
              st(rs_o, slot, hraw);
              unpack(hraw, v);  // GELU of the stored (rounded) pre-activation: what the backward's dGELU sees
            }
            // GELU_D stores no pre-activation: gelu and gelu' both come from the fp32 H here (no
            // round trip through 16 bits: 12 VALU instructions per 8 elements fewer)
            float gd[8];
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
              if constexpr (GELU_D) {
                f32x2 gv, gg;
                gelu_and_grad2(f32x2{v[e], v[e + 1]}, TANH, gv, gg);
                v[e] = gv[0];
                v[e + 1] = gv[1];
                gd[e] = gg[0];
                gd[e + 1] = gg[1];
              } else {
                const f32x2 gv = TANH ? gelu_tanh2(f32x2{v[e], v[e + 1]}) : gelu2(f32x2{v[e], v[e + 1]});
                v[e] = gv[0];
                v[e + 1] = gv[1];
              }
            }
            if constexpr (GELU_D) st(rs_o, slot, pack(gd));
          } else {
            float x[8];
            unpack(h == 0 ? ra[it] : rb[it], x);
            const bool ok = F || (wrow0 + lrow + 8 * slot < M && ncol < N);
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
              if constexpr (DGELU) {
                const f32x2 gg = TANH ? gelu_tanh_grad2(f32x2{x[e], x[e + 1]}) : gelu_grad2(f32x2{x[e], x[e + 1]});
                v[e] = ok ? v[e] * gg[0] : 0.f;
                v[e + 1] = ok ? v[e + 1] * gg[1] : 0.f;
              } else if constexpr (MUL) {
                v[e] = ok ? v[e] * x[e] : 0.f;
                v[e + 1] = ok ? v[e + 1] * x[e + 1] : 0.f;
              } else {
                v[e] += x[e];
                v[e + 1] += x[e + 1];
              }
            }
          }
          out = pack(v);
          if constexpr (COLSUM || Q8 != 0) {
            // fp16: the packed words are made opaque first. Left to see through pack -> unpack, hipcc (ROCm 7)
            // took elements 0 and 1 of the dGELU product from a v_fma_mixlo_f16 of their own (one rounding of
            // the product to fp16) next to the v_cvt_pk_f16_f32 of the fp32 product that is stored (two
            // roundings): the bias gradient then summed values that differ from the stored dh by an fp16 ulp
            // where the two disagree (persistent fp8 kernel with Q8 codes, edge-tile kernels)
            if constexpr (__is_same(T, f16)) asm("" : "+v"(out));
            float r[8];
            unpack(out, r);  // the bias grad / the fp8 codes take the stored (rounded) values
            if constexpr (COLSUM) {
#pragma unroll
              for (int e = 0; e < 8; ++e) csum[e] += r[e];
              // fp8 codes later, from LDS: the slot's chunk (read above, this lane's alone) takes the
              // stored value back — inline, the codes' live ranges spilled ~100 VGPRs in these variants
              if constexpr (Q8 != 0) {
                const int row = (HALVES ? it : slot) * 8 + lrow;
                *reinterpret_cast<u32x4*>(reg + row * 128 + (((lane & 7) ^ (row & 7)) << 4)) = out;
              }
            }
            if constexpr (Q8 != 0 && !COLSUM) {
              typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
              // edge tiles: a chunk past N holds column N - 1's sums under the last chunk's bias (clamped
              // staging, bias read at N - 8) — values of no element of C, kept out of max|C|
              const bool in_c = F || (wrow0 + lrow + 8 * slot < M && ncol < N);
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                q8mx = fmaxf(q8mx, in_c ? fabsf(r[e]) : 0.f);
                r[e] *= q8s;
              }
              const u32x2 w = u32x2{f8_pack4<Q8 - 1>(r[0], r[1], r[2], r[3]), f8_pack4<Q8 - 1>(r[4], r[5], r[6], r[7])};
              const int qr = lrow + slot * 8;
              const uint32_t qo = (F || (wrow0 + qr < M && ncol < N)) ? (uint32_t)(qr * ldc + lcol) : 0x80000000u;
              __builtin_amdgcn_raw_buffer_store_b64(w, rs_q, qo, 0, 0);
            }
          }
        }
        if constexpr (!(XD & kEpiCodesOnly)) st(rs_c, slot, out);
        // one slot at a time: unpacking every slot's operands up front (16 bf16 -> 16 fp32 per
        // slot, hoisted by the scheduler) is what pushed these epilogues past 256 VGPRs
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (HALVES && Q8 != 0 && COLSUM) {  // this half's stashed outputs -> fp8 codes
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll 4
        for (int it = 0; it < 8; ++it) {
          const int row = it * 8 + lrow;
          float r[8];
          unpack(*reinterpret_cast<const u32x4*>(reg + row * 128 + (((lane & 7) ^ (row & 7)) << 4)), r);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            q8mx = fmaxf(q8mx, fabsf(r[e]));
            r[e] *= q8s;
          }
          const u32x2 w = u32x2{f8_pack4<Q8 - 1>(r[0], r[1], r[2], r[3]), f8_pack4<Q8 - 1>(r[4], r[5], r[6], r[7])};
          __builtin_amdgcn_raw_buffer_store_b64(w, rs_q, (uint32_t)(((8 * h + it) * 8 + lrow) * ldc + lcol), 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr (COLSUM) {
      // lanes l, l^8, l^16, ... share the column chunk: reduce over the wave's 8 row slots
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float x = csum[e];
        x += __shfl_xor(x, 8, 64);
        x += __shfl_xor(x, 16, 64);
        x += __shfl_xor(x, 32, 64);
        csum[e] = x;
      }
      // waves wc = 0..3 of one wr cover disjoint columns: one partial row per (tile, wr)
      if (!(XD & kEpiNoStore) && lane < 8 && ncol < N) {
        float* pp = part + (int64_t)(tm * 2 + wr) * N + ncol;
        *reinterpret_cast<f32x4*>(pp) = f32x4{csum[0], csum[1], csum[2], csum[3]};
        *reinterpret_cast<f32x4*>(pp + 4) = f32x4{csum[4], csum[5], csum[6], csum[7]};
      }
    }
    if constexpr (Q8 != 0 && COLSUM && !HALVES) {  // the stashed outputs -> fp8 codes
      typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll 4
      for (int slot = 0; slot < 16; ++slot) {
        const int row = slot * 8 + lrow;
        float r[8];
        unpack(*reinterpret_cast<const u32x4*>(reg + row * 128 + (((lane & 7) ^ (row & 7)) << 4)), r);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          q8mx = fmaxf(q8mx, fabsf(r[e]));
          r[e] *= q8s;
        }
        const u32x2 w = u32x2{f8_pack4<Q8 - 1>(r[0], r[1], r[2], r[3]), f8_pack4<Q8 - 1>(r[4], r[5], r[6], r[7])};
        const uint32_t qo = (F || (wrow0 + row < M && ncol < N)) ? (uint32_t)(row * ldc + lcol) : 0x80000000u;
        __builtin_amdgcn_raw_buffer_store_b64(w, rs_q, qo, 0, 0);
      }
    }
    if constexpr (Q8 != 0 && HALVES) {
      *q8_defer = fmaxf(*q8_defer, q8mx);
    } else if constexpr (Q8 != 0) {  // one amax atomic per wave, filtered by a plain read (amax only grows)
      const float m = f8_wave_max(q8mx);
      if (lane == 0 && m > 0.f && m > *(volatile float*)q8.amax) f8_atomic_max_pos(q8.amax, m);
    }
  }
}


}  // namespace
}  // namespace apex
