// MXFP4 block-scaled NT GEMMs (apex.fp8.mx_gemm with an e2m1 operand) on gfx950's
// v_mfma_scale_f32_16x16x128_f8f6f4, beside the MXFP8 kernel of gemm_mx.hip:
//
//   C[m, n] = sum_k (A[m, k] * 2^(sa[m, k / 32] - 127)) * (B4[n, k] * 2^(sb[n, k / 32] - 127)) (+ bias[n])
//
//   fp4 x fp4   A [M, K / 2] and B4 [N, K / 2] packed e2m1 codes, K % 256 == 0
//   fp8 x fp4   A [M, K] e4m3 / e5m2 codes, B4 [N, K / 2] packed e2m1 codes, K % 128 == 0
//
// Packed e2m1: element 2 i of a row in the low nibble of byte i, element 2 i + 1 in the high nibble (the OCP
// float4_e2m1fn_x2 order); sa / sb [rows, K / 32] E8M0 bytes as in MXFP8. N % 8 == 0, every operand
// contiguous and 16-byte aligned; C is bf16, fp16 or fp32 from the fp32 accumulator. An fp4 A against an fp8
// B is not built.
//
// Instruction mapping, MEASURED on an MI355X with one wave, one-hot operands and a different scale per lane
// group (tests/test_mx4_gpu.py::test_placement pins it with integers). With l = 16 lk + lr:
//   * an fp4 operand (cbsz / blgp = 4) is 4 VGPRs: lane l holds row lr, K = 32 lk .. 32 lk + 31 in memory
//     order — VGPR v is bytes 4 v .. 4 v + 3 of the 16 packed bytes, the low nibble of a byte the even K. So
//     the hardware's nibble order is the public one (nothing is swapped while staging), and a lane's data is
//     ONE 32-block, lk — unlike an fp8 operand, whose 8 VGPRs are K = 16 lk .. + 15 and 64 + 16 lk .. + 15
//     (gemm_mx.hip);
//   * scales: as for fp8, the scale of block b of row lr is the opsel-selected byte of the scale VGPR of lane
//     16 b + lr — for an fp4 operand the lane that holds the block's data;
//   * mixed product: with the fp4 operand FIRST (cbsz 4) and the fp8 operand second (blgp 0 / 1) every
//     position pairs as stated above: fp8 K = 16 lk + i meets the fp4 lane group (16 lk + i) / 32, and both
//     operands' scales follow their own rule. The other order (fp8 first, fp4 second, cbsz 0 / blgp 4) paired
//     the positions the same way but returned sums that were no power of two for one-hot fp4 data with
//     per-block scales; it is not used;
//   * values: codes 0 .. 7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6, bit 3 the sign;
//   * a 0xFF scale byte on an fp4 operand behaves as gemm_mx.hip records for fp8: every output element of
//     that operand's row is NaN, whatever the block's codes (all-zero included), nothing else is touched —
//     in both products.
// The first source operand is the B fragment (as in gemm_mx.hip): D rows are N and a lane ends with
// C[m = lr][n = 4 lk .. 4 lk + 3]. B is the fp4 operand of both products, so the mixed product is in the
// measured-good order.
//
// Tiling. Workgroup = 512 threads = 8 waves, tile 256 (M) x 128 (N); wave (wid >> 1, wid & 1) owns 64 x 64 =
// 16 accumulator fragments. A K-tile is 128 bytes of every A row:
//   fp4 x fp4   256 K: A and B images are both 128-byte rows; the fragment of MFMA K-step h (K = 128 h ..) is
//               chunk 4 h + lk, so a lane reads chunks lk and lk + 4 — the two ds_read_b128 of gemm_mx.hip's
//               lds_frag — and feeds them to two MFMAs instead of one: 32 MFMAs per wave and barrier where
//               MXFP8 has 16, for the same LDS and global bytes. Eight scale bytes per row and K-tile: two
//               dwords, staged as two planes [h][row].
//   fp8 x fp4   128 K: A as in gemm_mx.hip; B rows are 64 bytes (4 chunks), a lane reads chunk lk with one
//               ds_read_b128; one scale dword per row.
// 256 x 256 for fp4 x fp4 was reconsidered and not taken: at 256 K per tile three stages need 204 KB of
// LDS (160 KB exist); at 128 K per tile it fits, but the 128 accumulator VGPRs plus 12 fragments leave one
// wave per SIMD and every barrier covers half the MFMAs. The compiler's register figures are in
// profiles/README.md (no scratch in any instantiation).
//
// LDS: three stages of {A 32 KB, B 16 / 8 KB, A scales 2 / 1 KB, B scales 1 / 0.5 KB} = 153 / 124.5 KB (the
// epilogue images need 136 KB, which sizes the mixed kernel's array). Codes and scales arrive by
// global_load_lds two K-tiles ahead, issued at the top of an iteration; every wave issues the same number of
// pieces per K-tile (fp4 x fp4: 4 A + 2 B + 2 scale = 8; mixed: 4 A + 1 B + 1 scale = 6; waves 6 and 7 repeat
// the B-scale pieces of waves 4 and 5), so `s_waitcnt vmcnt(pieces)` at the bottom retires K-tile t + 1 and
// leaves t + 2 in flight; one raw s_barrier per K-tile (gemm_mx.hip's RAW / WAR argument, unchanged).
//
// Swizzle and banks. 128-byte rows: chunk c of row r at slot c ^ ((r >> 1) & 7), gemm_mx.hip's argument.
// 64-byte rows (the mixed product's B): that mapping would put rows r and r + 4 — the same 64 banks — on
// slots that differ in bit 1 of r only, i.e. 16 lanes on 8 slots. Here chunk c of row r is at slot
// c ^ ((r >> 2) & 3). A b128 read is served 16 lanes at a time: lr = 0 .. 15 at one lk, the same logical chunk
// c of 16 consecutive rows r = 4 q + i. Byte address = 256 q + 64 i + 16 (c ^ q): within the 256-byte span of
// the 64 banks the lane's 16-byte unit is 4 i + (c ^ q); for one i the four q give four different c ^ q, and
// different i lie in different quarters: 16 lanes, 16 different units, no conflict, for every c.
//
// Epilogue (none / bias) and tile order (XCD remap, panels of 8 M-tiles): gemm_mx.hip's.
#include "gemm_kernels.h"

namespace apex {
namespace {

constexpr int X4_BM = 256, X4_BN = 128, X4_THREADS = 512, X4_GROUP_M = 8;
constexpr int X4_EPI_LD = 68;                               // fp32 row stride of a wave's epilogue image
constexpr int X4_EPI_BYTES = 8 * 64 * X4_EPI_LD * 4;

// FA: hardware format of the A operand (0 = e4m3, 1 = e5m2, 4 = e2m1); B is e2m1
template <int FA>
struct X4 {
  static constexpr bool A4 = FA == 4;
  static constexpr int KT = A4 ? 256 : 128;                 // K per K-tile
  static constexpr int NS = A4 ? 2 : 1;                     // MFMA K-steps = scale dwords per row and K-tile
  static constexpr int B_ROW = A4 ? 128 : 64;               // bytes of a B row per K-tile
  static constexpr int B_PIECES = X4_BN * B_ROW / 1024 / 8; // 1 KB pieces of B per wave: 2 / 1
  static constexpr int A_BYTES = X4_BM * 128, B_BYTES = X4_BN * B_ROW;
  static constexpr int SA_OFF = A_BYTES + B_BYTES;          // A scales: NS planes of one dword per row
  static constexpr int SB_OFF = SA_OFF + NS * X4_BM * 4;
  static constexpr int STAGE = SB_OFF + NS * X4_BN * 4;
  static constexpr int PIECES = 4 + B_PIECES + NS;          // global_load_lds per wave and K-tile
  static constexpr int LDS = 3 * STAGE > X4_EPI_BYTES ? 3 * STAGE : X4_EPI_BYTES;
  static_assert(LDS <= 160 * 1024, "LDS of one workgroup");
};

__device__ __forceinline__ void x4_glds4(const void* g, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, 0);
}

// chunk c (16 bytes = 32 K) of row r of a 64-byte-row image
__device__ __forceinline__ s16x8 x4_frag64(const char* tile, int r, int c) {
  return *reinterpret_cast<const s16x8*>(tile + r * 64 + ((c ^ ((r >> 2) & 3)) << 4));
}

// b: the fp4 B fragment (first source); a0 (, a1): the A fragment, fp4 (a0 alone) or fp8 (chunks lk, lk + 4)
template <int FA>
__device__ __forceinline__ f32x4 x4_mfma(const s16x8& b, const s16x8& a0, const s16x8& a1, int sb, int sa, const f32x4& c) {
  const i32x4 xb = __builtin_bit_cast(i32x4, b), xa0 = __builtin_bit_cast(i32x4, a0), xa1 = __builtin_bit_cast(i32x4, a1);
  const i32x8 bv = __builtin_shufflevector(xb, xb, 0, 1, 2, 3, -1, -1, -1, -1);
  if constexpr (FA == 4) {
    const i32x8 av = __builtin_shufflevector(xa0, xa0, 0, 1, 2, 3, -1, -1, -1, -1);
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bv, av, c, 4, 4, 0, sb, 0, sa);
  } else {
    const i32x8 av = __builtin_shufflevector(xa0, xa1, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bv, av, c, 4, FA, 0, sb, 0, sa);
  }
}

// Per-lane global addresses of the pieces a wave stages per K-tile, at K-tile 0 (rows past the operand's last
// are read from its last row: they only feed outputs the epilogue does not store)
template <int FA>
struct X4Src {
  const uint8_t* a[4];
  const uint8_t* b[X4<FA>::B_PIECES];
  const uint8_t* s;
};

template <int FA>
__device__ __forceinline__ X4Src<FA> x4_src(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                            const uint8_t* __restrict__ SA, const uint8_t* __restrict__ SB, int M, int N,
                                            int K, int m0, int n0, int wid, int lane) {
  using G = X4<FA>;
  X4Src<FA> p;
  const int64_t lda = G::A4 ? (K >> 1) : K, ldb = K >> 1;   // row strides in bytes
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = (wid * 4 + j) * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((r >> 1) & 7);
    p.a[j] = A + (int64_t)min(m0 + r, M - 1) * lda + chunk * 16;
  }
  if constexpr (G::A4) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = (wid * 2 + j) * 8 + (lane >> 3);
      const int chunk = (lane & 7) ^ ((r >> 1) & 7);
      p.b[j] = B + (int64_t)min(n0 + r, N - 1) * ldb + chunk * 16;
    }
  } else {  // 64-byte rows: a piece is 16 rows of 4 chunks
    const int r = wid * 16 + (lane >> 2);
    const int chunk = (lane & 3) ^ ((r >> 2) & 3);
    p.b[0] = B + (int64_t)min(n0 + r, N - 1) * ldb + chunk * 16;
  }
  const int64_t sk = K >> 5;
  if (wid < 4) p.s = SA + (int64_t)min(m0 + wid * 64 + lane, M - 1) * sk;
  else p.s = SB + (int64_t)min(n0 + (wid & 1) * 64 + lane, N - 1) * sk;
  return p;
}

// K-tile t -> stage image `st`
template <int FA>
__device__ __forceinline__ void x4_stage(const X4Src<FA>& p, int t, char* st, int wid) {
  using G = X4<FA>;
#pragma unroll
  for (int j = 0; j < 4; ++j) glds16(p.a[j] + t * 128, st + (wid * 4 + j) * 1024);
#pragma unroll
  for (int j = 0; j < G::B_PIECES; ++j)
    glds16(p.b[j] + t * G::B_ROW, st + G::A_BYTES + (wid * G::B_PIECES + j) * 1024);
#pragma unroll
  for (int h = 0; h < G::NS; ++h)
    x4_glds4(p.s + (t * G::NS + h) * 4, st + (wid < 4 ? G::SA_OFF + h * X4_BM * 4 + wid * 256
                                                      : G::SB_OFF + h * X4_BN * 4 + (wid & 1) * 256));
}

template <typename T, int FA>
__global__ void __launch_bounds__(X4_THREADS) gemm_mx4_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                              const uint8_t* __restrict__ SA,
                                                              const uint8_t* __restrict__ SB, T* __restrict__ C,
                                                              const T* __restrict__ bias, int M, int N, int K) {
  using G = X4<FA>;
  __shared__ __attribute__((aligned(16))) char smem[G::LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 1, wc = wid & 1;
  const int lr = lane & 15, lk = lane >> 4;

  // ---- tile: XCD remap, then GROUP_M panels ----
  const int tiles_m = (M + X4_BM - 1) / X4_BM, tiles_n = (N + X4_BN - 1) / X4_BN;
  const int wg = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int group = X4_GROUP_M * tiles_n;
  const int first_m = (wg / group) * X4_GROUP_M;
  const int gm = min(tiles_m - first_m, X4_GROUP_M);
  const int m0 = (first_m + (wg % group) % gm) * X4_BM, n0 = ((wg % group) / gm) * X4_BN;

  f32x4 acc[4][4];  // [N block j][M block i]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nt = K / G::KT;
  const X4Src<FA> src = x4_src<FA>(A, B, SA, SB, M, N, K, m0, n0, wid, lane);
  x4_stage<FA>(src, 0, smem, wid);
  if (nt > 1) {
    x4_stage<FA>(src, 1, smem + G::STAGE, wid);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G::PIECES) : "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  bar();

  int s0 = 0, s2 = 2 * G::STAGE;  // byte offsets of the stages of K-tiles t and t + 2
  const int sh = 8 * lk;
  for (int t = 0; t < nt; ++t) {
    if (t + 2 < nt) x4_stage<FA>(src, t + 2, smem + s2, wid);
    const char* st = smem + s0;
    s16x8 fa[4][2], fb[4][G::NS];
    int sa[4][G::NS], sb[4][G::NS];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = wc * 64 + j * 16 + lr;
#pragma unroll
      for (int h = 0; h < G::NS; ++h) {
        fb[j][h] = G::A4 ? lds_frag(st + G::A_BYTES, r, lk + 4 * h) : x4_frag64(st + G::A_BYTES, r, lk);
        sb[j][h] = (int)(reinterpret_cast<const uint32_t*>(st + G::SB_OFF)[h * X4_BN + r] >> sh);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = wr * 64 + i * 16 + lr;
      fa[i][0] = lds_frag(st, r, lk);
      fa[i][1] = lds_frag(st, r, lk + 4);
#pragma unroll
      for (int h = 0; h < G::NS; ++h) sa[i][h] = (int)(reinterpret_cast<const uint32_t*>(st + G::SA_OFF)[h * X4_BM + r] >> sh);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int h = 0; h < G::NS; ++h)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[j][i] = x4_mfma<FA>(fb[j][h], fa[i][G::A4 ? h : 0], fa[i][1], sb[j][h], sa[i][h], acc[j][i]);
    __builtin_amdgcn_s_setprio(0);
    if (t + 2 < nt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G::PIECES) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bar();
    s2 = s0;  // stage (t + 3) % 3 = t % 3
    s0 = s0 + G::STAGE == 3 * G::STAGE ? 0 : s0 + G::STAGE;
  }

  // ---- epilogue: every wave is past its last operand read (the loop's last barrier) ----
  float* img = reinterpret_cast<float*>(smem) + wid * 64 * X4_EPI_LD;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(img + (i * 16 + lr) * X4_EPI_LD + j * 16 + 4 * lk) = acc[j][i];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's own writes, read back by other lanes
  const int cn = (lane & 7) * 8, n = n0 + wc * 64 + cn;
  if (n >= N) return;  // (N % 8 == 0: a lane's 8 columns are all inside or all outside)
  float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (bias) {
    float lo[4], hi[4];
    load_f<T, 4>(bias + n, lo);
    load_f<T, 4>(bias + n + 4, hi);
#pragma unroll
    for (int k = 0; k < 4; ++k) bv[k] = lo[k], bv[4 + k] = hi[k];
  }
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int rr = it * 8 + (lane >> 3), m = m0 + wr * 64 + rr;
    const f32x4 lo = *reinterpret_cast<const f32x4*>(img + rr * X4_EPI_LD + cn);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(img + rr * X4_EPI_LD + cn + 4);
    if (m >= M) continue;
    const float o0[4] = {lo[0] + bv[0], lo[1] + bv[1], lo[2] + bv[2], lo[3] + bv[3]};
    const float o1[4] = {hi[0] + bv[4], hi[1] + bv[5], hi[2] + bv[6], hi[3] + bv[7]};
    T* dst = C + (int64_t)m * N + n;
    store_f<T, 4>(dst, o0);
    store_f<T, 4>(dst + 4, o1);
  }
}

template <typename T>
int launch_mx4(const MxGemmArgs& g, hipStream_t s) {
  const int tiles = ((g.M + X4_BM - 1) / X4_BM) * ((g.N + X4_BN - 1) / X4_BN);
#define APEX_MX4_LAUNCH(FA)                                                                                       \
  hipLaunchKernelGGL((gemm_mx4_kernel<T, FA>), dim3(tiles), dim3(X4_THREADS), 0, s, g.A, g.B, g.SA, g.SB, (T*)g.C, \
                     (const T*)g.bias, g.M, g.N, g.K)
  switch (g.fmt_a) {
    case 0: APEX_MX4_LAUNCH(0); break;
    case 1: APEX_MX4_LAUNCH(1); break;
    default: APEX_MX4_LAUNCH(4); break;
  }
#undef APEX_MX4_LAUNCH
  return (int)hipGetLastError();
}

}  // namespace

bool gemm_mx4_supported(int64_t M, int64_t N, int64_t K, int fmt_a) {
  const int64_t kt = fmt_a == 2 ? 256 : 128;
  if (fmt_a < 0 || fmt_a > 2 || M < 1 || N < 8 || K < kt || K % kt || (N & 7)) return false;
  if (M >= (1ll << 31) - X4_BM || N >= (1ll << 31) - X4_BN || K >= (1ll << 31)) return false;
  const int64_t tiles = ((M + X4_BM - 1) / X4_BM) * ((N + X4_BN - 1) / X4_BN);
  return tiles < (1ll << 31);
}

int gemm_mx4(const MxGemmArgs& g, int out_dt, hipStream_t s) {
  if (g.fmt_b != 2 || !gemm_mx4_supported(g.M, g.N, g.K, g.fmt_a)) return -2;
  APEX_DISPATCH_T(out_dt, T, return launch_mx4<T>(g, s));
  return -1;
}

}  // namespace apex
