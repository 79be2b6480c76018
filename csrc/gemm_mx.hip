// MXFP8 block-scaled NT GEMM (apex.fp8.mx_gemm) on gfx950's v_mfma_scale_f32_16x16x128_f8f6f4:
//
//   C[m, n] = sum_k (A8[m, k] * 2^(sa[m, k / 32] - 127)) * (B8[n, k] * 2^(sb[n, k / 32] - 127)) (+ bias[n])
//
// A8 [M, K] and B8 [N, K] are OCP e4m3 / e5m2 codes, sa [M, K / 32] and sb [N, K / 32] E8M0 bytes (the
// OCP Microscaling 1 x 32 block format, csrc/mx.hip writes both). K % 128 == 0, N % 8 == 0, every
// operand contiguous; C is bf16, fp16 or fp32 from the fp32 accumulator. No alpha: MX has no
// per-tensor factor. The per-tensor fp8 kernel (gemm.hip) stays as it is: its 256 x 256 loop sits at the
// 256-VGPR limit and has no register left for scales, so MX is a kernel of its own.
//
// Instruction mapping, MEASURED on an MI355X with one K = 128 tile and a different scale on each of its
// four blocks (tests/test_mx_gpu.py::test_scale_placement pins it with integers). With l = 16 lk + lr:
//   * operand data: lane l holds row lr; its VGPRs 0 .. 3 are K = 16 lk .. 16 lk + 15 and its VGPRs
//     4 .. 7 are K = 64 + 16 lk .. 64 + 16 lk + 15, in memory order. A lane's 32 values therefore belong
//     to TWO 32-blocks, lk >> 1 and 2 + (lk >> 1) — not to one block, as a reading of the instruction's
//     description as "32 consecutive K per lane" would have it (a first version of this kernel fed each
//     lane K = 32 lk .. 32 lk + 31 and got, for data in block 0 alone, half of it scaled by block 0's
//     scale and half by block 2's);
//   * scales: the scale of block b (K = 32 b .. 32 b + 31) of row lr is the opsel-selected byte of the
//     scale VGPR of lane 16 b + lr. Lane l thus supplies byte lk of its row's scale dword of the K-tile,
//     although its own data lies in other blocks.
// So the fragment is chunks lk and lk + 4 of the 128-byte K row — the pairing gemm_mainloop.h already
// uses, which makes the instruction's K the memory K — and the kernel reads the row's scale dword and
// shifts it right by 8 lk (one VALU per 16-row fragment and K-tile; opsel is an immediate, the same byte
// in every lane, so a lane cannot select "byte lk" by opsel), opsel 0.
// The first source operand is the B fragment ("swapped" product, as in gemm.hip): D rows are then N and
// a lane ends with C[m = lr][n = 4 lk .. 4 lk + 3], four consecutive columns.
// A scale byte of 0xFF (E8M0 NaN, what mx_quantize writes for a block holding an inf or a NaN), measured:
// the hardware honours it. Every output element whose A row or B row has a 0xFF block is NaN, whatever
// the block's codes (all-zero codes included) and whatever the other operand's scale; other elements are
// untouched. 0xFE is the finite 2^127.
//
// Tiling. Workgroup = 512 threads = 8 waves, tile 256 (M) x 128 (N), K-tile 128 bytes; wave (wr, wc) =
// (wid >> 1, wid & 1) owns 64 x 64: 16 accumulator fragments (64 VGPRs), 4 + 4 operand fragments of
// two 16-byte chunks (64 VGPRs), 8 scale VGPRs, 14 staging addresses. No scratch, 166 VGPRs in every
// instantiation (the compiler's figures, profiles/README.md), so two waves per SIMD. The 256 x 256 / 128 x 64
// geometry of gemm.hip does not fit: it sits at 256 VGPRs before the scales.
//
// LDS: three stages of {A 32 KB, B 16 KB, A scales 1 KB, B scales 512 B} = 148.5 KB. Every K-tile's
// codes and scales arrive by global_load_lds (16-byte pieces for the codes as in gemm_mainloop.h, one
// 4-byte piece per wave for the scales: lane = row, its dword = the row's four block scales of this
// K-tile), issued two K-tiles ahead at the top of an iteration, i.e. outside the MFMA section; the
// public scale layout stays [rows, K / 32]. Every wave issues exactly 7 pieces per K-tile (4 A, 2 B, 1
// scale; waves 6 and 7 repeat the B-scale pieces of waves 4 and 5, same bytes to the same place), so
// `s_waitcnt vmcnt(7)` at the bottom retires K-tile t + 1 and leaves t + 2 in flight; one raw s_barrier
// per K-tile makes it visible and frees stage (t - 1) % 3 for the next issue (WAR: that stage's last
// reads were waited for by lgkmcnt(0) before the previous barrier).
//
// Swizzle and bank conflicts. The image of an operand tile is gemm_mainloop.h's: 128-byte rows, chunk c
// of row r at slot c ^ ((r >> 1) & 7); a lane reads chunks lk and lk + 4 with two ds_read_b128 (lds_frag).
// Argument over banks: the hardware serves a b128 read 16 consecutive lanes at a time (256 bytes = all
// 64 banks once); such a group is lr = 0 .. 15 at one lk, so all 16 lanes ask for the same logical chunk
// c of 16 consecutive rows. Rows 2q and 2q + 1 lie in different halves of the 64 banks (row stride 128
// bytes), and over the 8 row pairs (r >> 1) & 7 takes 8 different values, so c ^ ((r >> 1) & 7) takes 8
// different slots: 16 lanes, 16 different 4-bank groups, no conflict, for every c. It is the read pattern
// for which gemm_mainloop.h records zero LDS bank conflicts under rocprof. The scale reads are
// ds_read_b32 of 16 consecutive dwords, the same 16 in each of the four lk groups (broadcast).
//
// Epilogue: none or bias. Each wave writes its 64 x 64 fp32 accumulators to its own 17 KB of the (now
// idle) LDS and reads them back row-wise, so that a lane stores 8 consecutive columns (16 bytes of bf16)
// and a wave 8 rows x 128 bytes per instruction instead of 16 rows x 8 bytes.
//
// Tile order: gemm_kernels.h's bijective XCD remap, then panels of 8 M-tiles walked down one N column.
#include "gemm_kernels.h"

namespace apex {
namespace {

constexpr int MX_BM = 256, MX_BN = 128, MX_THREADS = 512, MX_GROUP_M = 8;
constexpr int MX_A_BYTES = MX_BM * 128;                     // 32 KB of codes
constexpr int MX_B_BYTES = MX_BN * 128;                     // 16 KB
constexpr int MX_SA_OFF = MX_A_BYTES + MX_B_BYTES;          // A scales: one dword per row
constexpr int MX_SB_OFF = MX_SA_OFF + MX_BM * 4;            // B scales
constexpr int MX_STAGE_BYTES = MX_SB_OFF + MX_BN * 4;       // 50688
constexpr int MX_LDS_BYTES = 3 * MX_STAGE_BYTES;            // 152064 <= 160 KB
constexpr int MX_EPI_LD = 68;                               // fp32 row stride of a wave's epilogue image
static_assert(8 * 64 * MX_EPI_LD * 4 <= MX_LDS_BYTES, "epilogue images fit the staging LDS");

__device__ __forceinline__ void glds4(const void* g, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, 0);
}

// FA / FB: formats of the first / second source operand (0 = e4m3, 1 = e5m2); sa / sb: their scale
// bytes in bits 0 .. 7 of the lane's VGPR
template <int FA, int FB>
__device__ __forceinline__ f32x4 mfma_mx(const s16x8 (&a)[2], const s16x8 (&b)[2], int sa, int sb, const f32x4& c) {
  const i32x4 a0 = __builtin_bit_cast(i32x4, a[0]), a1 = __builtin_bit_cast(i32x4, a[1]);
  const i32x4 b0 = __builtin_bit_cast(i32x4, b[0]), b1 = __builtin_bit_cast(i32x4, b[1]);
  const i32x8 av = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
  const i32x8 bv = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, c, FA, FB, 0, sa, 0, sb);
}

// Per-lane global addresses of the 7 pieces a wave stages per K-tile, at K-tile 0 (rows past the operand's
// last are read from its last row: they only feed outputs the epilogue does not store)
struct MxSrc {
  const uint8_t* a[4];
  const uint8_t* b[2];
  const uint8_t* s;
};

__device__ __forceinline__ MxSrc mx_src(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                        const uint8_t* __restrict__ SA, const uint8_t* __restrict__ SB, int M, int N,
                                        int K, int m0, int n0, int wid, int lane) {
  MxSrc p;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = (wid * 4 + j) * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((r >> 1) & 7);
    const int gr = min(m0 + r, M - 1);
    p.a[j] = A + (int64_t)gr * K + chunk * 16;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = (wid * 2 + j) * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((r >> 1) & 7);
    const int gr = min(n0 + r, N - 1);
    p.b[j] = B + (int64_t)gr * K + chunk * 16;
  }
  const int64_t sk = K >> 5;
  if (wid < 4) p.s = SA + (int64_t)min(m0 + wid * 64 + lane, M - 1) * sk;
  else p.s = SB + (int64_t)min(n0 + (wid & 1) * 64 + lane, N - 1) * sk;
  return p;
}

__device__ __forceinline__ int mx_next(int s) { return s + MX_STAGE_BYTES == MX_LDS_BYTES ? 0 : s + MX_STAGE_BYTES; }

// K-tile t -> stage image `st`
__device__ __forceinline__ void mx_stage(const MxSrc& p, int t, char* st, int wid) {
  const int k0 = t * 128;
#pragma unroll
  for (int j = 0; j < 4; ++j) glds16(p.a[j] + k0, st + (wid * 4 + j) * 1024);
#pragma unroll
  for (int j = 0; j < 2; ++j) glds16(p.b[j] + k0, st + MX_A_BYTES + (wid * 2 + j) * 1024);
  glds4(p.s + t * 4, st + (wid < 4 ? MX_SA_OFF + wid * 256 : MX_SB_OFF + (wid & 1) * 256));
}

template <typename T, int FA, int FB>
__global__ void __launch_bounds__(MX_THREADS) gemm_mx_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                             const uint8_t* __restrict__ SA,
                                                             const uint8_t* __restrict__ SB, T* __restrict__ C,
                                                             const T* __restrict__ bias, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) char smem[MX_LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 1, wc = wid & 1;
  const int lr = lane & 15, lk = lane >> 4;

  // ---- tile: XCD remap, then GROUP_M panels ----
  const int tiles_m = (M + MX_BM - 1) / MX_BM, tiles_n = (N + MX_BN - 1) / MX_BN;
  const int wg = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int group = MX_GROUP_M * tiles_n;
  const int first_m = (wg / group) * MX_GROUP_M;
  const int gm = min(tiles_m - first_m, MX_GROUP_M);
  const int m0 = (first_m + (wg % group) % gm) * MX_BM, n0 = ((wg % group) / gm) * MX_BN;

  f32x4 acc[4][4];  // [N block j][M block i]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nt = K >> 7;
  const MxSrc src = mx_src(A, B, SA, SB, M, N, K, m0, n0, wid, lane);
  mx_stage(src, 0, smem, wid);
  if (nt > 1) {
    mx_stage(src, 1, smem + MX_STAGE_BYTES, wid);
    asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  bar();

  int s0 = 0;  // byte offset of K-tile t's stage (t % 3); K-tile t + 2 goes to stage (t + 2) % 3
  const int sh = 8 * lk;
  for (int t = 0; t < nt; ++t) {
    if (t + 2 < nt) mx_stage(src, t + 2, smem + mx_next(mx_next(s0)), wid);
    const char* st = smem + s0;
    s16x8 fa[4][2], fb[4][2];
    int sa[4], sb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = wc * 64 + j * 16 + lr;
      fb[j][0] = lds_frag(st + MX_A_BYTES, r, lk);
      fb[j][1] = lds_frag(st + MX_A_BYTES, r, lk + 4);
      sb[j] = (int)(reinterpret_cast<const uint32_t*>(st + MX_SB_OFF)[r] >> sh);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = wr * 64 + i * 16 + lr;
      fa[i][0] = lds_frag(st, r, lk);
      fa[i][1] = lds_frag(st, r, lk + 4);
      sa[i] = (int)(reinterpret_cast<const uint32_t*>(st + MX_SA_OFF)[r] >> sh);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[j][i] = mfma_mx<FB, FA>(fb[j], fa[i], sb[j], sa[i], acc[j][i]);
    __builtin_amdgcn_s_setprio(0);
    if (t + 2 < nt) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bar();
    s0 = mx_next(s0);
  }

  // ---- epilogue: every wave is past its last operand read (the loop's last barrier) ----
  float* img = reinterpret_cast<float*>(smem) + wid * 64 * MX_EPI_LD;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(img + (i * 16 + lr) * MX_EPI_LD + j * 16 + 4 * lk) = acc[j][i];
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
    const f32x4 lo = *reinterpret_cast<const f32x4*>(img + rr * MX_EPI_LD + cn);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(img + rr * MX_EPI_LD + cn + 4);
    if (m >= M) continue;
    const float o0[4] = {lo[0] + bv[0], lo[1] + bv[1], lo[2] + bv[2], lo[3] + bv[3]};
    const float o1[4] = {hi[0] + bv[4], hi[1] + bv[5], hi[2] + bv[6], hi[3] + bv[7]};
    T* dst = C + (int64_t)m * N + n;
    store_f<T, 4>(dst, o0);
    store_f<T, 4>(dst + 4, o1);
  }
}

template <typename T>
int launch_mx(const MxGemmArgs& g, hipStream_t s) {
  const int tiles = ((g.M + MX_BM - 1) / MX_BM) * ((g.N + MX_BN - 1) / MX_BN);
#define APEX_MX_LAUNCH(FA, FB)                                                                                     \
  hipLaunchKernelGGL((gemm_mx_kernel<T, FA, FB>), dim3(tiles), dim3(MX_THREADS), 0, s, g.A, g.B, g.SA, g.SB, (T*)g.C, \
                     (const T*)g.bias, g.M, g.N, g.K)
  switch (g.fmt_a * 2 + g.fmt_b) {
    case 0: APEX_MX_LAUNCH(0, 0); break;
    case 1: APEX_MX_LAUNCH(0, 1); break;
    case 2: APEX_MX_LAUNCH(1, 0); break;
    default: APEX_MX_LAUNCH(1, 1); break;
  }
#undef APEX_MX_LAUNCH
  return (int)hipGetLastError();
}

}  // namespace

bool gemm_mx_supported(int64_t M, int64_t N, int64_t K) {
  if (M < 1 || N < 8 || K < 128 || (K & 127) || (N & 7)) return false;
  if (M >= (1ll << 31) - MX_BM || N >= (1ll << 31) - MX_BN || K >= (1ll << 31)) return false;
  const int64_t tiles = ((M + MX_BM - 1) / MX_BM) * ((N + MX_BN - 1) / MX_BN);
  return tiles < (1ll << 31);
}

int gemm_mx(const MxGemmArgs& g, int out_dt, hipStream_t s) {
  if (!gemm_mx_supported(g.M, g.N, g.K) || (g.fmt_a | g.fmt_b) & ~1) return -2;
  APEX_DISPATCH_T(out_dt, T, return launch_mx<T>(g, s));
  return -1;
}

}  // namespace apex
