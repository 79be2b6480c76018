// MFMA GEMM (gemm.hip), device side 1 of 3: tile constants, global -> LDS staging, MFMA fragments and
// the two K-loop schedules. Included by gemm_epilogue.h / gemm_kernels.h; the tiling is described at
// the top of gemm.hip. Everything here is internal to the including translation unit (gemm.hip, or a
// lab under tools/gemmlab).
#pragma once
#include "common.h"
#include "kernels.h"

namespace apex {
namespace {

// Lab switches: the kernels' template argument DBG, 0 in every production instantiation; the labs
// (tools/gemmlab) instantiate the kernels with sums of these to time one part of a kernel without
// the others. The values are those of the labs' recorded command lines and profiles.
constexpr int kLabNoGlds = 32;       // K loop issues no global -> LDS copies (the prologue's still run)
constexpr int kLabNoBarrier = 64;    // K loop without its barriers
constexpr int kLabNoDsRead = 128;    // K loop without its fragment ds_reads
constexpr int kLabNoEpilogue = 512;  // gemm_nt_kernel: accumulators kept live, nothing stored
constexpr int kLabOldLoop = 1024;    // gemm_nt_kernel: mainloop_bk64 where production runs mainloop_bal
constexpr int kLabTrace = 2048;      // per-workgroup timeline record (trace_record, gemm_kernels.h)
constexpr int kLabEpiShift = 12;     // gemm_persist_kernel: DBG bits 12, 13 are its epilogue's XD bits 0, 1
// (bits 1 .. 16 and 256 belong to the lab-only kernels of tools/gemmlab/lab_variants.h)

// G_GROUP_M: M-tiles per panel of the tile order (consecutive workgroups walk GROUP_M M-tiles down
// one N column before moving right); APEX_G_GROUP_M overrides it at build time (lab sweeps)
#ifndef APEX_G_GROUP_M
#define APEX_G_GROUP_M 8
#endif
constexpr int GB_M = 256, GB_N = 256, GB_K = 64, G_THREADS = 512, G_GROUP_M = APEX_G_GROUP_M;
constexpr int G_TILE_BYTES = GB_M * GB_K * 2;       // one operand tile: 32 KB
constexpr int G_BUF_BYTES = 2 * G_TILE_BYTES;       // A + B: 64 KB
constexpr int G_LDS_BYTES = 2 * G_BUF_BYTES;        // double buffered: 128 KB

typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename T> __device__ __forceinline__ f32x4 mfma16(const s16x8& a, const s16x8& b, const f32x4& c);
template <> __device__ __forceinline__ f32x4 mfma16<bf16>(const s16x8& a, const s16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4 mfma16<f16>(const s16x8& a, const s16x8& b, const f32x4& c) {
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  return __builtin_amdgcn_mfma_f32_16x16x32_f16((h8)a, (h8)b, c, 0, 0, 0);
}

// FP8 (gfx950 f8f6f4 block-scaled MFMA, 16x16x128, 2x the bf16 rate): the 32 bytes of a lane's
// operand are the SAME two 16-byte LDS chunks the bf16 path reads for its two 16x16x32 K-steps
// (chunks lk and lk + 4 of the 128-byte K-tile row). The K order inside the instruction is thus a
// permutation of the tile's K, identical for both operands, so the dot products are unchanged and
// the LDS reads stay conflict-free. Block scales are all 2^0 (E8M0 127): the per-tensor scales
// are applied in the epilogue (alpha). Formats: 0 = e4m3 (OCP fn), 1 = e5m2.
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
template <int FMT_A, int FMT_B>
__device__ __forceinline__ f32x4 mfma_f8(const s16x8& a0, const s16x8& a1, const s16x8& b0, const s16x8& b1,
                                         const f32x4& c) {
  const i32x4 xa0 = __builtin_bit_cast(i32x4, a0), xa1 = __builtin_bit_cast(i32x4, a1);
  const i32x4 xb0 = __builtin_bit_cast(i32x4, b0), xb1 = __builtin_bit_cast(i32x4, b1);
  const i32x8 a = __builtin_shufflevector(xa0, xa1, 0, 1, 2, 3, 4, 5, 6, 7);
  const i32x8 b = __builtin_shufflevector(xb0, xb1, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FMT_A, FMT_B, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
}

// the lane id computed afresh (volatile: never CSE'd with an earlier copy or hoisted out of a loop), so
// no VGPR holding it — or an address derived from it — stays live across a K loop: the fp8 main loop
// runs at the 256-VGPR limit, and in the persistent kernel one more live register spills inside it
__device__ __forceinline__ int lane_id_fresh() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

__device__ __forceinline__ void glds16(const void* g, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ s16x8 lds_frag(const char* tile, int r, int c) {
  return *reinterpret_cast<const s16x8*>(tile + r * 128 + ((c ^ ((r >> 1) & 7)) << 4));
}

__device__ __forceinline__ void bar() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// One operand K-tile = 32 glds pieces of 1 KB; wave `wid` owns pieces wid*4 .. wid*4+3 and
// stage_pieces issues pieces [p0, p0+2) of them.
//  TR = false (operand [rows][K], K contiguous): piece = 8 rows x 128 B of K; image [256 rows][64 K],
//    chunk c of row r at c ^ ((r >> 1) & 7).
//  TR = true (operand stored [K][rows], rows contiguous — the weight-gradient GEMM, where the
//    contraction runs over tokens): piece = 2 K-rows x 512 B; image [64 K][256 rows], chunk c of
//    K-row r at c ^ ftr(r); fragments are gathered with ds_read_b64_tr_b16 (hardware transpose).
//    fp8 (the fp8 weight gradient): K-tile = 128 K-rows of 256 B, piece = 4 K-rows, chunk c of
//    K-row r at c ^ ftr8(r); fragments from ds_read_b64_tr_b8.
__device__ __forceinline__ int ftr(int r) { return 2 * (r & 3) + 8 * ((r >> 3) & 1); }
// A tr_b8 read's 32-lane half covers K-rows r0 + q and r0 + 16 + q (q = 0..7, r0 % 8 == 0), 8 bytes
// each of one 16-byte chunk: (r & 7) | bit 4 of r puts those 16 rows on 16 distinct slots (64 banks)
__device__ __forceinline__ int ftr8(int r) { return (r & 7) | (((r >> 4) & 1) << 3); }

template <typename T, bool TR>
__device__ __forceinline__ void stage_pieces(const T* __restrict__ g, int64_t ld, int row0, int rows, int k0,
                                             char* lds_tile, int wid, int lane, int p0) {
#pragma unroll
  for (int j = p0; j < p0 + 2; ++j) {
    const int piece = wid * 4 + j;
    static_assert(!TR, "TR = true stages through TrSrc (below)");
    const int r = piece * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((r >> 1) & 7);
    int gr = row0 + r;
    gr = gr < rows ? gr : rows - 1;
    glds16(g + (int64_t)gr * ld + k0 + chunk * (16 / (int)sizeof(T)), lds_tile + piece * 1024);
  }
}

// TR = true staging: lane l of piece p reads g + (k0 + r) * ld + col, r = the piece's K-row of the lane,
// col = the swizzled chunk's first column. Only k0 changes over the K loop and it is wave-uniform, so the
// address is split and the loop carries no per-lane address math (formed whole per load it cost seven
// VALU, three of them 32-bit multiplies, for each of the 16 loads of a K-tile pair, all in the R sections
// the other wave group's MFMA phase has to cover):
//   off[j]  per lane, loop invariant: byte offset of piece j's 16-byte chunk from the first K-row this
//           wave stages in a K-tile — the K-row inside the wave's four pieces, the swizzled chunk column
//           and the partial-tile clamp. 32 bits: gemm_tt*_supported bound ld so that the wave's 8
//           (fp8: 16) K-rows span less than 4 GiB.
//   base    wave-uniform 64-bit address of that K-row in the K-tile staged last: SGPRs, the saddr form of
//           global_load_lds, advanced by `step` bytes with scalar adds (operands past 4 GiB: nothing
//           running is 32 bits wide). It moves only when the next K-tile exists, so no address outside
//           [g, g + K * ld) is ever formed.
template <typename T>
struct TrSrc {
  const char* base;
  int64_t step;
  uint32_t off[4];
};
template <typename T>
__device__ __forceinline__ TrSrc<T> tr_src(const T* __restrict__ g, int64_t ld, int row0, int rows, int wid, int lane) {
  constexpr int ES = (int)sizeof(T), LPR = 16 * ES, RPP = 64 / LPR;  // K-rows per piece: 2 (16-bit), 4 (fp8)
  TrSrc<T> s;
  s.base = reinterpret_cast<const char*>(g + (int64_t)(wid * 4 * RPP) * ld);
  s.step = (int64_t)(128 / ES) * ld * ES;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = (wid * 4 + j) * RPP + lane / LPR;
    const int chunk = (lane % LPR) ^ (ES == 1 ? ftr8(r) : ftr(r));
    // partial tiles (rows % 256, e.g. GPT-2's 1600 / 4800): chunks past the last row read the
    // last full chunk instead (rows % 8 == 0) — they only feed output rows / columns the
    // bounds-checked epilogue does not store, and the last K-row never reads past the tensor
    int col = row0 + chunk * (16 / ES);
    col = col < rows ? col : rows - 16 / ES;
    s.off[j] = ((uint32_t)(j * RPP + lane / LPR) * (uint32_t)ld + (uint32_t)col) * (uint32_t)ES;
  }
  return s;
}
template <typename T>
__device__ __forceinline__ void stage_tr(const TrSrc<T>& s, char* lds_tile, int wid, int p0) {
#pragma unroll
  for (int j = p0; j < p0 + 2; ++j) {
    // kept opaque so that the zero-extension stays in the block of the load: hoisted out of the K loop,
    // hipcc carries each offset as a 64-bit VGPR pair and adds the base per lane (v_lshl_add_u64)
    // instead of selecting the saddr form
    uint32_t o = s.off[j];
    asm volatile("" : "+v"(o));
    glds16(s.base + o, lds_tile + (wid * 4 + j) * 1024);
  }
}
// One K-loop staging step: stage_pieces for TR = false (ts unused); for TR the operand's TrSrc, moved to
// the next K-tile first when `adv` (the first two of its four pieces)
template <typename T, bool TR>
__device__ __forceinline__ void stage_k(const T* __restrict__ g, int64_t ld, int row0, int rows, int k0, char* lds_tile,
                                        int wid, int lane, int p0, TrSrc<T>* ts, bool adv) {
  if constexpr (TR) {
    if (adv) ts->base += ts->step;
    stage_tr(*ts, lds_tile, wid, p0);
  } else {
    stage_pieces<T, false>(g, ld, row0, rows, k0, lds_tile, wid, lane, p0);
  }
}

typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ s16x4 lds_tr16(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}
typedef int i32x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ i32x2v lds_tr8(const char* p) {
  return __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2v*)(p));
}

// MFMA fragment for tile rows rb .. rb+15, K step s (32 wide): lane holds rows rb + lr,
// K = 32s + 8 lk .. +7. ES = operand element bytes (1: fp8, where the 16 bytes are K = 64s + 16lk ..
// +15, the chunk 4s + lk the NT image's lds_frag reads — see mfma_f8).
template <bool TR, int ES = 2>
__device__ __forceinline__ s16x8 frag(const char* tile, int rb, int s, int lr, int lk) {
  if constexpr (TR && ES == 1) {
    // two 8(K) x 16(rows) byte blocks (ds_read_b64_tr_b8): lane 2q+p of a 16-lane group addresses
    // K-row 64s + 16lk + 8h + q, rows rb + 8p .. +7; it receives row rb + lr, K-rows 8h .. 8h+7
    const int q = lr >> 1, pp = lr & 1;
    const int cl = rb >> 4;
    const int r0 = s * 64 + 16 * lk + q, r1 = r0 + 8;
    const i32x2v lo = lds_tr8(tile + r0 * 256 + ((cl ^ ftr8(r0)) << 4) + pp * 8);
    const i32x2v hi = lds_tr8(tile + r1 * 256 + ((cl ^ ftr8(r1)) << 4) + pp * 8);
    return __builtin_bit_cast(s16x8, i32x4{lo[0], lo[1], hi[0], hi[1]});
  } else if constexpr (TR) {
    // two 4(K) x 16(rows) transposed blocks: lane 4q+p of a 16-lane group addresses K-row
    // 32s + 8lk + 4h + q, rows rb + 4p .. +3; it receives row rb + lr, K 4h .. 4h+3
    const int q = lr >> 2, pp = lr & 3;
    const int cl = (rb >> 3) + (pp >> 1);
    const int r0 = s * 32 + 8 * lk + q, r1 = r0 + 4;
    const s16x4 lo = lds_tr16(tile + r0 * 512 + ((cl ^ ftr(r0)) << 4) + (pp & 1) * 8);
    const s16x4 hi = lds_tr16(tile + r1 * 512 + ((cl ^ ftr(r1)) << 4) + (pp & 1) * 8);
    return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  } else {
    return lds_frag(tile, rb + lr, s * 4 + lk);
  }
}

// Main loop schedule ("ping-pong", cdna_hip_programming.md §5 256² template, own phase plan):
// the 8 waves form two groups by M half (wr); group 1 runs one barrier behind group 0, so in
// every barrier interval one group issues its 16 MFMAs while the other issues its LDS reads
// and global->LDS copies on the same SIMDs. Per K-tile and wave, four phases, each
//   R: ds_read subtile, 2 glds pieces, [vmcnt], lgkmcnt(0)  | barrier
//   M: 16 x mfma_16x16x32 (one 64x32 quadrant, K = 64)      | barrier
//     p1  R: A rows mh=0 (8 frags) + B cols nh=0 (4)   stage A(t+1) pieces 0,1 -> other buffer
//     p2  R: B cols nh=1 (4)                           stage A(t+1) pieces 2,3
//     p3  R: A rows mh=1 (8)                           stage B(t+2) pieces 0,1 -> this buffer
//     p4  R: -                                         stage B(t+2) pieces 2,3; vmcnt(4)
//     quadrants (mh,nh): p1 (0,0)  p2 (0,1)  p3 (1,1)  p4 (1,0)
// WAR: B of this buffer is last read in p2 and A in p3; lgkmcnt(0) before each barrier retires
// the reads, so restaging one phase later (B(t+2) in p3) is safe; A(t+1) goes to the buffer whose
// A was last read in the previous tile's p3. RAW: vmcnt(4) in p4 retires everything but B(t+2)
// (i.e. A(t+1), B(t+1)) before the barrier that precedes the next tile's first read.
// Measured alternatives (profiles/r1_gemm_ksweep_variants.jsonl, same box, interleaved): LDS wait
// after the barrier with the glds moved to p2/p4 — within 1 %; BK = 32 with four buffers and one
// 32-MFMA phase per K-tile (half the barriers, loads 3 tiles ahead) — 12-15 % slower (the glds
// issue then sits inside the MFMA section); 256x128 tiles at two workgroups per CU (BK 32, three
// stages, no ping-pong; profiles/r1_gemm_*_2wg_variant.jsonl) — its epilogue does overlap the
// other workgroup's MFMAs (K = 64: 55 vs 65 us at N = 4096) but the main loop is ~60 % slower;
// two phases per K-tile with the whole tile read in the first R section (half the barriers, next
// loads 4 sections ahead, 256 VGPRs; profiles/r1_gemm_ksweep_2phase.jsonl) — within 1 %; the two
// glds pieces of each phase issued from inside the MFMA section (after 8 of its 16 MFMAs) instead
// of the R section, same buffers and waits (vmcnt(2) in R4) — 5-7 % slower on every BERT shape
// at M = 98304 (profiles/r2_gemm_glds_in_mma_ab.jsonl, same box).
// hipBLASLt's kernel on the same shape (rocprof): one wave per SIMD with 128x128 wave tiles (256
// AGPR accumulators), 74 % MFMA busy vs 64 % here. That geometry in HIP source (fragments
// software-pipelined under 64-MFMA halves) makes hipcc shuffle ~220 accumulator copies
// (v_accvgpr_read/write) per K-tile through the loop-carried phis, so it is not used. rocprof on the 32768x1024x4096 case: MFMA busy 65 %
// of SIMD cycles at 1.98 GHz, zero LDS bank conflicts.
//
// Prologue of both schedules (gemm_nt_kernel; the persistent kernel keeps its own copy, see there):
// A(0), B(0) -> buffer 0, B(1) -> buffer 1 when there is a second K-tile; tile 0 retired (B(1)'s four
// pieces stay in flight) and visible to every wave; then the wave groups staggered
template <typename T, bool TR>
__device__ __forceinline__ void mainloop_prologue(const T* __restrict__ A, const T* __restrict__ B, int M, int N,
                                                  int nt, int64_t lda, int64_t ldb, int m0, int n0, char* smem,
                                                  int wid, int wr, int lane, TrSrc<T>* ts) {
  constexpr int BKE = 128 / (int)sizeof(T);
  stage_k<T, TR>(A, lda, m0, M, 0, smem, wid, lane, 0, &ts[0], false);
  stage_k<T, TR>(A, lda, m0, M, 0, smem, wid, lane, 2, &ts[0], false);
  stage_k<T, TR>(B, ldb, n0, N, 0, smem + G_TILE_BYTES, wid, lane, 0, &ts[1], false);
  stage_k<T, TR>(B, ldb, n0, N, 0, smem + G_TILE_BYTES, wid, lane, 2, &ts[1], false);
  if (nt > 1) {
    stage_k<T, TR>(B, ldb, n0, N, BKE, smem + G_BUF_BYTES + G_TILE_BYTES, wid, lane, 0, &ts[1], true);
    stage_k<T, TR>(B, ldb, n0, N, BKE, smem + G_BUF_BYTES + G_TILE_BYTES, wid, lane, 2, &ts[1], false);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  bar();
  if (wr == 1) bar();  // stagger group 1 by one barrier
}

template <typename T, bool TR, int FA, int FB, int DBG, bool FRESH = false>
__device__ __forceinline__ void mainloop_bk64_loop(const T* __restrict__ A, const T* __restrict__ B, int M, int N,
                                                   int K, int64_t lda, int64_t ldb, int m0, int n0, char* smem,
                                                   int wid, int wr, int wc, int lane, f32x4 (&acc)[4][8],
                                                   TrSrc<T>* ts = nullptr);
template <typename T, bool TR, int FA = -1, int FB = -1, int DBG = 0>
__device__ __forceinline__ void mainloop_bk64(const T* __restrict__ A, const T* __restrict__ B, int M, int N, int K,
                                              int64_t lda, int64_t ldb, int m0, int n0, char* smem, int wid, int wr,
                                              int wc, int lane, f32x4 (&acc)[4][8]) {
  // one K-tile = 128 bytes of every row: 64 bf16/f16 elements or 128 fp8 ones
  constexpr bool F8 = FA >= 0;
  static_assert(!F8 || sizeof(T) == 1, "fp8: uint8 codes");
  constexpr int BKE = 128 / (int)sizeof(T);
  const int nt = K / BKE;
  TrSrc<T> ts[2];
  if constexpr (TR) {
    ts[0] = tr_src<T>(A, lda, m0, M, wid, lane);
    ts[1] = tr_src<T>(B, ldb, n0, N, wid, lane);
  }
  mainloop_prologue<T, TR>(A, B, M, N, nt, lda, ldb, m0, n0, smem, wid, wr, lane, ts);
  mainloop_bk64_loop<T, TR, FA, FB, DBG>(A, B, M, N, K, lda, ldb, m0, n0, smem, wid, wr, wc, lane, acc, ts);
}

// mainloop_bk64's K loop (tile 0 staged and retired, the wave groups staggered): also the fp8 body of
// the persistent kernel, which sets FRESH: the LDS-DMA source addresses are recomputed from a fresh
// lane id every K-tile instead of being kept in 16 VGPRs across the loop (there they spilled, and each
// reload waited, in vmcnt order, for every load and store in flight)
template <typename T, bool TR, int FA, int FB, int DBG, bool FRESH>
__device__ __forceinline__ void mainloop_bk64_loop(const T* __restrict__ A, const T* __restrict__ B, int M, int N,
                                                   int K, int64_t lda, int64_t ldb, int m0, int n0, char* smem,
                                                   int wid, int wr, int wc, int lane_in, f32x4 (&acc)[4][8],
                                                   TrSrc<T>* ts) {
  constexpr bool F8 = FA >= 0;
  constexpr int BKE = 128 / (int)sizeof(T);
  const int nt = K / BKE;
  const int lr = lane_in & 15, lk = lane_in >> 4;
  s16x8 fa[4][2], fb0[2][2], fb1[2][2];
  for (int t = 0; t < nt; ++t) {
    const int lane = FRESH ? lane_id_fresh() : lane_in;
    char* cur = smem + (t & 1) * G_BUF_BYTES;
    char* oth = smem + ((t + 1) & 1) * G_BUF_BYTES;
    const char* ta = cur;
    const char* tb = cur + G_TILE_BYTES;
    const bool ld_a = t + 1 < nt, ld_b = t + 2 < nt;
    // ---------------- p1: A mh=0, B nh=0; stage A(t+1) pieces 0,1 ----------------
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if constexpr (!(DBG & kLabNoDsRead)) for (int s = 0; s < 2; ++s) fb0[j][s] = frag<TR, sizeof(T)>(tb, wc * 64 + j * 16, s, lr, lk);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if constexpr (!(DBG & kLabNoDsRead)) for (int s = 0; s < 2; ++s) fa[i][s] = frag<TR, sizeof(T)>(ta, wr * 128 + i * 16, s, lr, lk);
    if (ld_a && !(DBG & kLabNoGlds)) stage_k<T, TR>(A, lda, m0, M, (t + 1) * BKE, oth, wid, lane, 0, &ts[0], true);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (!(DBG & kLabNoBarrier)) bar();
    __builtin_amdgcn_s_setprio(1);
    if constexpr (F8) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = mfma_f8<FB, FA>(fb0[j][0], fb0[j][1], fa[i][0], fa[i][1], acc[j][i]);
    } else {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = mfma16<T>(fb0[j][s], fa[i][s], acc[j][i]);
    }
    __builtin_amdgcn_s_setprio(0);
    if constexpr (!(DBG & kLabNoBarrier)) bar();
    // ---------------- p2: B nh=1; stage A(t+1) pieces 2,3 ----------------
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if constexpr (!(DBG & kLabNoDsRead)) for (int s = 0; s < 2; ++s) fb1[j][s] = frag<TR, sizeof(T)>(tb, wc * 64 + 32 + j * 16, s, lr, lk);
    if (ld_a && !(DBG & kLabNoGlds)) stage_k<T, TR>(A, lda, m0, M, (t + 1) * BKE, oth, wid, lane, 2, &ts[0], false);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (!(DBG & kLabNoBarrier)) bar();
    __builtin_amdgcn_s_setprio(1);
    if constexpr (F8) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[2 + j][i] = mfma_f8<FB, FA>(fb1[j][0], fb1[j][1], fa[i][0], fa[i][1], acc[2 + j][i]);
    } else {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[2 + j][i] = mfma16<T>(fb1[j][s], fa[i][s], acc[2 + j][i]);
    }
    __builtin_amdgcn_s_setprio(0);
    if constexpr (!(DBG & kLabNoBarrier)) bar();
    // ---------------- p3: A mh=1; stage B(t+2) pieces 0,1 into this buffer ----------------
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if constexpr (!(DBG & kLabNoDsRead)) for (int s = 0; s < 2; ++s) fa[i][s] = frag<TR, sizeof(T)>(ta, wr * 128 + 64 + i * 16, s, lr, lk);
    if (ld_b && !(DBG & kLabNoGlds)) stage_k<T, TR>(B, ldb, n0, N, (t + 2) * BKE, cur + G_TILE_BYTES, wid, lane, 0, &ts[1], true);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (!(DBG & kLabNoBarrier)) bar();
    __builtin_amdgcn_s_setprio(1);
    if constexpr (F8) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[2 + j][4 + i] = mfma_f8<FB, FA>(fb1[j][0], fb1[j][1], fa[i][0], fa[i][1], acc[2 + j][4 + i]);
    } else {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[2 + j][4 + i] = mfma16<T>(fb1[j][s], fa[i][s], acc[2 + j][4 + i]);
    }
    __builtin_amdgcn_s_setprio(0);
    if constexpr (!(DBG & kLabNoBarrier)) bar();
    // ---------------- p4: stage B(t+2) pieces 2,3; retire A(t+1), B(t+1) ----------------
    if (ld_b) {
      if constexpr (!(DBG & kLabNoGlds)) stage_k<T, TR>(B, ldb, n0, N, (t + 2) * BKE, cur + G_TILE_BYTES, wid, lane, 2, &ts[1], false);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if constexpr (!(DBG & kLabNoBarrier)) bar();
    __builtin_amdgcn_s_setprio(1);
    if constexpr (F8) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][4 + i] = mfma_f8<FB, FA>(fb0[j][0], fb0[j][1], fa[i][0], fa[i][1], acc[j][4 + i]);
    } else {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][4 + i] = mfma16<T>(fb0[j][s], fa[i][s], acc[j][4 + i]);
    }
    __builtin_amdgcn_s_setprio(0);
    if constexpr (!(DBG & kLabNoBarrier)) bar();
  }
}

// ---- "balanced" variant of the same schedule: the production main loop (kLabOldLoop selects the
// one above, for lab A/B) ----------------------------------------------------------------------------
// The loop above reads 12 fragments in p1, 4 in p2, 8 in p3 and none in p4; p1's read section is the
// long pole of the ping-pong (the other group's 16-MFMA section has to cover it). Here the quadrant
// order alternates per K-tile — even tiles (0,0) (0,1) (1,1) (1,0), odd tiles (0,1) (0,0) (1,0) (1,1)
// — so the B half a tile starts with is the one its predecessor ended without, and p4 reads it from
// the other buffer for the next tile: 8 / 4 / 8 / 4 fragments per phase. That needs B(t+1) landed
// one phase earlier: p3 waits for it (vmcnt(6): only A(t+1) and B(t+2)'s first pieces stay in
// flight), and the barriers after p3 make it visible. WAR is unchanged: B(t+1) is last read in
// tile t+1's p2, before B(t+3) is staged over it in p3. Measured against the loop above
// (profiles/r4_gemm_balanced_loop.jsonl, same box, interleaved, outputs bit-identical): NT 8192^3
// 1.49 -> 1.53 PF/s, BERT M = 98304 shapes 1-5 % faster (FFN2 dgrad + residual 642 -> 618 us);
// transposed-read weight gradients 2-8 % (two ds_read_b64_tr_b16 per fragment: the read sections
// are longer there, so evening them out pays more).
template <bool TR, int ES = 2>
__device__ __forceinline__ void read_fa(s16x8 (&fa)[4][2], const char* ta, int rb, int lr, int lk) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int s = 0; s < 2; ++s) fa[i][s] = frag<TR, ES>(ta, rb + i * 16, s, lr, lk);
}
template <bool TR, int ES = 2>
__device__ __forceinline__ void read_fb(s16x8 (&fb)[2][2], const char* tb, int cb, int lr, int lk) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int s = 0; s < 2; ++s) fb[j][s] = frag<TR, ES>(tb, cb + j * 16, s, lr, lk);
}
template <typename T, int FA, int FB, int MH, int NH>
__device__ __forceinline__ void quad_mma(f32x4 (&acc)[4][8], const s16x8 (&fa)[4][2], const s16x8 (&fb)[2][2]) {
  __builtin_amdgcn_s_setprio(1);
  if constexpr (FA >= 0) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[2 * NH + j][4 * MH + i] = mfma_f8<FB, FA>(fb[j][0], fb[j][1], fa[i][0], fa[i][1], acc[2 * NH + j][4 * MH + i]);
  } else {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[2 * NH + j][4 * MH + i] = mfma16<T>(fb[j][s], fa[i][s], acc[2 * NH + j][4 * MH + i]);
  }
  __builtin_amdgcn_s_setprio(0);
}

template <typename T, bool TR, int FA, int FB, int DBG, int PAR>
__device__ __forceinline__ void bal_tile(int t, int nt, const T* __restrict__ A, const T* __restrict__ B, int M, int N,
                                         int64_t lda, int64_t ldb, int m0, int n0, char* smem, int wid, int wr, int wc,
                                         int lane, f32x4 (&acc)[4][8], s16x8 (&fa)[4][2], s16x8 (&fb)[2][2][2],
                                         TrSrc<T>* ts = nullptr) {
  constexpr int BKE = 128 / (int)sizeof(T);
  constexpr int OP = 1 - PAR;
  const int lr = lane & 15, lk = lane >> 4;
  // t & 1 == PAR, but kept opaque (an SGPR the compiler cannot fold): with a constant buffer base
  // per parity hipcc keeps separate fragment-address registers for both buffers and spills
  int pb = t & 1;
  asm("" : "+s"(pb));
  char* cur = smem + pb * G_BUF_BYTES;
  char* oth = smem + (pb ^ 1) * G_BUF_BYTES;
  const char* ta = cur;
  const char* tb = cur + G_TILE_BYTES;
  const bool ld_a = t + 1 < nt, ld_b = t + 2 < nt;
  constexpr bool RD = !(DBG & kLabNoDsRead), GL = !(DBG & kLabNoGlds), BR = !(DBG & kLabNoBarrier);
  // p1: A rows mh=0; stage A(t+1) pieces 0,1
  if constexpr (RD) read_fa<TR, sizeof(T)>(fa, ta, wr * 128, lr, lk);
  if (GL && ld_a) stage_k<T, TR>(A, lda, m0, M, (t + 1) * BKE, oth, wid, lane, 0, &ts[0], true);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if constexpr (BR) bar();
  quad_mma<T, FA, FB, 0, PAR>(acc, fa, fb[PAR]);
  if constexpr (BR) bar();
  // p2: B half OP; stage A(t+1) pieces 2,3
  if constexpr (RD) read_fb<TR, sizeof(T)>(fb[OP], tb, wc * 64 + OP * 32, lr, lk);
  if (GL && ld_a) stage_k<T, TR>(A, lda, m0, M, (t + 1) * BKE, oth, wid, lane, 2, &ts[0], false);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if constexpr (BR) bar();
  quad_mma<T, FA, FB, 0, OP>(acc, fa, fb[OP]);
  if constexpr (BR) bar();
  // p3: A rows mh=1; stage B(t+2) pieces 0,1 into this buffer; retire B(t+1) for p4
  if constexpr (RD) read_fa<TR, sizeof(T)>(fa, ta, wr * 128 + 64, lr, lk);
  if (ld_b) {
    if constexpr (GL) stage_k<T, TR>(B, ldb, n0, N, (t + 2) * BKE, cur + G_TILE_BYTES, wid, lane, 0, &ts[1], true);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  } else if (ld_a) {
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if constexpr (BR) bar();
  quad_mma<T, FA, FB, 1, OP>(acc, fa, fb[OP]);
  if constexpr (BR) bar();
  // p4: next tile's first B half (OP) from the other buffer; stage B(t+2) pieces 2,3; retire A(t+1).
  // (Unconditional: after the last tile it reads stale LDS that nothing uses — a conditional load
  // would keep the old fragment live across the phase and cost registers.)
  if constexpr (RD) read_fb<TR, sizeof(T)>(fb[OP], oth + G_TILE_BYTES, wc * 64 + OP * 32, lr, lk);
  if (ld_b) {
    if constexpr (GL) stage_k<T, TR>(B, ldb, n0, N, (t + 2) * BKE, cur + G_TILE_BYTES, wid, lane, 2, &ts[1], false);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if constexpr (BR) bar();
  quad_mma<T, FA, FB, 1, PAR>(acc, fa, fb[PAR]);
  if constexpr (BR) bar();
}

template <typename T, bool TR, int FA = -1, int FB = -1, int DBG = 0>
__device__ __forceinline__ void mainloop_bal(const T* __restrict__ A, const T* __restrict__ B, int M, int N, int K,
                                             int64_t lda, int64_t ldb, int m0, int n0, char* smem, int wid, int wr,
                                             int wc, int lane, f32x4 (&acc)[4][8]) {
  constexpr int BKE = 128 / (int)sizeof(T);
  const int nt = K / BKE;
  TrSrc<T> ts[2];
  if constexpr (TR) {
    ts[0] = tr_src<T>(A, lda, m0, M, wid, lane);
    ts[1] = tr_src<T>(B, ldb, n0, N, wid, lane);
  }
  mainloop_prologue<T, TR>(A, B, M, N, nt, lda, ldb, m0, n0, smem, wid, wr, lane, ts);
  s16x8 fa[4][2], fb[2][2][2];
  const int lr = lane & 15, lk = lane >> 4;
  if constexpr (!(DBG & kLabNoDsRead)) read_fb<TR, sizeof(T)>(fb[0], smem + G_TILE_BYTES, wc * 64, lr, lk);  // tile 0's first B half
  int t = 0;
  for (; t + 1 < nt; t += 2) {
    bal_tile<T, TR, FA, FB, DBG, 0>(t, nt, A, B, M, N, lda, ldb, m0, n0, smem, wid, wr, wc, lane, acc, fa, fb, ts);
    bal_tile<T, TR, FA, FB, DBG, 1>(t + 1, nt, A, B, M, N, lda, ldb, m0, n0, smem, wid, wr, wc, lane, acc, fa, fb, ts);
  }
  if (t < nt) bal_tile<T, TR, FA, FB, DBG, 0>(t, nt, A, B, M, N, lda, ldb, m0, n0, smem, wid, wr, wc, lane, acc, fa, fb, ts);
}

}  // namespace
}  // namespace apex
