// MFMA GEMM (gemm.hip), device side 3 of 3: the workgroup -> tile map and the kernels — one tile per
// workgroup (gemm_nt_kernel: NT and transposed-read, 16-bit and fp8), persistent (gemm_persist_kernel),
// and the 2-D transpose. The launchers are in gemm.hip.
#pragma once
#include "gemm_epilogue.h"

namespace apex {
namespace {

// Launch control word (gemm_nt_kernel's argument `ctl`, no device-variable load in the kernel):
//   bits 0..14  first-round stagger units (experiment, off by default): half of the first round's
//               workgroups (bid & 8) sleep `units` x s_sleep(127) before starting (gemm.hip host_stagger)
//   bit 15      kCtlSplitXcd: split-major XCD remap of split-K (transposed-read) launches
//   bits 16..   diagnostics mode, gemm_set_dbg(): 2 = skip the epilogue (main-loop-only timing)
constexpr int kCtlSplitXcd = 0x8000;

// Timeline record of one workgroup / tile (kLabTrace, both kernels): the 100 MHz real-time clock at its
// start (tr0), after the main loop (tr1) and after the epilogue's stores completed, plus HW_ID / XCC_ID
__device__ __forceinline__ void trace_record(uint64_t* tp, uint64_t tr0, uint64_t tr1, int tid) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  bar();
  const uint64_t tr2 = __builtin_amdgcn_s_memrealtime();
  if (tid == 0) {
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    tp[0] = tr0;
    tp[1] = tr1;
    tp[2] = tr2;
    tp[3] = (uint64_t)hw | ((uint64_t)xcc << 32);
  }
}

// XCD remap: workgroups are dealt to the 8 XCDs round-robin; id v of n -> a position such that each XCD
// walks one contiguous range of the n positions (bijective for any n)
__device__ __forceinline__ int xcd_remap(int v, int n) {
  const int xcd = v & 7, q = n >> 3, rr = n & 7;
  return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (v >> 3);
}
// GROUP_M panel order: position wg (after the XCD remap) -> tile (tm, tn) and its origin (m0, n0)
__device__ __forceinline__ void panel_coords(int wg, int tiles_m, int tiles_n, int& m0, int& n0, int& tm) {
  const int group = G_GROUP_M * tiles_n;
  const int first_m = (wg / group) * G_GROUP_M;
  const int gm = min(tiles_m - first_m, G_GROUP_M);
  tm = first_m + (wg % group) % gm;
  const int tn = (wg % group) / gm;
  m0 = tm * GB_M;
  n0 = tn * GB_N;
}

// T: output / epilogue dtype; TI: operand dtype (T, or uint8_t fp8 with formats FA (A) / FB (B) and
// the dequantisation alpha = alpha_a[0] * alpha_b[0] read on the device)
template <typename T, int EPI, bool TR, bool EDGE, typename TI = T, int FA = -1, int FB = -1, int DBG = 0,
          int Q8 = 0, bool NOC = false>
__global__ void __launch_bounds__(G_THREADS) gemm_nt_kernel(const TI* __restrict__ A, const TI* __restrict__ B,
                                                            T* __restrict__ C, int M, int N, int K, int64_t lda,
                                                            int64_t ldb, int64_t ldc, const T* __restrict__ bias,
                                                            const T* __restrict__ aux, int64_t ldaux,
                                                            T* __restrict__ aux_out, float* __restrict__ part,
                                                            int ctl, const float* __restrict__ alpha_a = nullptr,
                                                            const float* __restrict__ alpha_b = nullptr,
                                                            Q8Out q8 = Q8Out{}) {
  __shared__ __attribute__((aligned(16))) char smem[G_LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;
  const int lr = lane & 15, lk = lane >> 4;

  // ---- tile mapping: bijective XCD remap, then GROUP_M panel order ----
  const int tiles_m = (M + GB_M - 1) / GB_M, tiles_n = (N + GB_N - 1) / GB_N;
  const int nwg = tiles_m * tiles_n;
  const int bid = blockIdx.x;
  int wg, split = TR ? (int)blockIdx.y : 0;
  if (TR && (ctl & kCtlSplitXcd) && gridDim.y > 1) {
    // split-K: the remap runs over (split, tile) jointly in dispatch order, split-major, so the
    // workgroups an XCD holds share one K-range and meet each other's A / B panels in its L2 (tile-
    // major, each dY panel of a weight gradient was streamed by every XCD holding one of its tiles)
    const int v = xcd_remap(bid + nwg * (int)blockIdx.y, nwg * (int)gridDim.y);
    split = v / nwg;
    wg = v - split * nwg;
  } else {
    wg = xcd_remap(bid, nwg);
  }
  int m0, n0, tm;
  panel_coords(wg, tiles_m, tiles_n, m0, n0, tm);

  f32x4 acc[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  // kLabTrace (lab timeline trace, bf16 kernels only): per workgroup the 100 MHz real-time clock at
  // start, after the main loop and after the epilogue's stores completed, plus HW_ID / XCC_ID, into
  // the uint64 buffer passed as alpha_a (unused by the 16-bit kernels)
  uint64_t tr0 = 0, tr1 = 0;
  if constexpr (DBG & kLabTrace) tr0 = __builtin_amdgcn_s_memrealtime();

  {
    const int st = ctl & 0x7fff;
    if (st > 0 && bid < 256 && (bid & 8)) {
      for (int i = 0; i < st; ++i) __builtin_amdgcn_s_sleep(127);
    }
  }
  if constexpr (TR) {
    // split-K slice of the transposed-read launches: K = ALL contraction rows, cut into gridDim.y slices
    // of whole K-tiles, [split * T / S, (split + 1) * T / S) for T K-tiles (the slices differ by at most
    // one K-tile: any slice count fills the CUs, e.g. BERT's QKV weight gradient, 48 tiles, at 5 slices
    // = 240 workgroups where 4 gave 192)
    constexpr int BKT = 128 / (int)sizeof(TI);  // rows per K-tile (64 16-bit, 128 fp8)
    const int nkt = K / BKT, ns = (int)gridDim.y;
    const int kb = (int)((int64_t)split * nkt / ns), ke = (int)((int64_t)(split + 1) * nkt / ns);
    A += (int64_t)kb * BKT * lda;
    B += (int64_t)kb * BKT * ldb;
    K = (ke - kb) * BKT;
  }
  // mainloop_bal for the 16-bit kernels; the fp8 instantiations and the edge-tile dGELU / multiply
  // epilogues keep the previous schedule (their epilogues hold more registers: the balanced loop's
  // extra live fragment spilled 50-240 VGPRs in fp8, 2 -> 52 in edge EPI_MUL). kLabOldLoop forces
  // the previous one (lab A/B).
  constexpr bool EDGE_HEAVY = EDGE && epi_colsum(EPI);
  if constexpr ((DBG & kLabOldLoop) || FA >= 0 || EDGE_HEAVY)
    mainloop_bk64<TI, TR, FA, FB, DBG>(A, B, M, N, K, lda, ldb, m0, n0, smem, wid, wr, wc, lane, acc);
  else
    mainloop_bal<TI, TR, FA, FB, DBG>(A, B, M, N, K, lda, ldb, m0, n0, smem, wid, wr, wc, lane, acc);
  if (wr == 0) bar();  // re-align the groups
  bar();               // every wave is past its last ds_read: LDS is free for the epilogue
  if constexpr (DBG & kLabTrace) tr1 = __builtin_amdgcn_s_memrealtime();
  if constexpr (EPI == EPI_F32) {
    // fp32 slab (split-K partials): each lane stores its 4 consecutive columns per fragment
    // (fp8 operands: dequantised here, alpha = the two per-tensor inverse scales)
    float* out = part + (int64_t)split * M * ldc;
    float sc = 1.f;
    if constexpr (FA >= 0) sc = alpha_a[0] * alpha_b[0];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wc * 64 + j * 16 + 4 * lk;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int m = m0 + wr * 128 + i * 16 + lr;
        if (m < M && n < N) *reinterpret_cast<f32x4*>(out + (int64_t)m * ldc + n) = acc[j][i] * sc;
      }
    }
    return;
  }
  if constexpr (EPI == EPI_F32_ACC) {
    // part[m, n] += acc in fp32 (one K slice: gemm_tt_acc's main_grad accumulation), in two halves
    // of 16 fragments whose 16-byte loads are all issued before the first add
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      f32x4 prev[2][8];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int n = n0 + wc * 64 + (2 * hf + jj) * 16 + 4 * lk;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int m = m0 + wr * 128 + i * 16 + lr;
          prev[jj][i] = m < M && n < N ? *reinterpret_cast<const f32x4*>(part + (int64_t)m * ldc + n) : f32x4{};
        }
      }
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int n = n0 + wc * 64 + (2 * hf + jj) * 16 + 4 * lk;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int m = m0 + wr * 128 + i * 16 + lr;
          if (m < M && n < N) *reinterpret_cast<f32x4*>(part + (int64_t)m * ldc + n) = prev[jj][i] + acc[2 * hf + jj][i];
        }
      }
    }
    return;
  }

  if (__builtin_expect((ctl >> 16) == 2, 0) || (DBG & kLabNoEpilogue)) {  // keep the accumulators live, store nothing
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 8; ++i) t += acc[j][i][0] + acc[j][i][1] + acc[j][i][2] + acc[j][i][3];
    if (t == 1.2345e-30f) C[0] = from_f<T>(t);
    return;
  }
  float alpha = 1.f;
  if constexpr (FA >= 0) alpha = alpha_a[0] * alpha_b[0];
  epilogue<T, EPI, EDGE, 0, 4, false, Q8, false, NoHook, NOC ? kEpiCodesOnly : 0>(
      acc, smem + wid * 16384, C, M, N, ldc, bias, aux, ldaux, aux_out, part, m0, n0, tm, wr, wc, lane, alpha, q8);
  if constexpr ((DBG & kLabTrace) && FA < 0) trace_record((uint64_t*)alpha_a + (int64_t)bid * 4, tr0, tr1, tid);
}


// ============================================================================================
// Persistent kernel: one workgroup per CU walks the tile list; the next tile's first K-tile is
// loaded while this tile's epilogue runs.
//
// The timeline trace of the one-tile-per-workgroup kernel (tools/gemmlab LAB_TRACE,
// profiles/r5_gemm_trace_m98304.jsonl) puts 3.2-11.4 us of epilogue and ~0.5 us of dispatch gap
// after each 25-28 us main loop at K = 1024, and the main loop itself includes the prologue: the
// first K-tile's 64 KB arriving while every CU's new workgroup asks for its own at once. Here the
// workgroup, after its last main-loop read of LDS:
//   1. issues the NEXT tile's A(0) and B(0) (buffer 0, 64 KB) — they load during the epilogue;
//   2. runs the epilogue with its accumulators staged through buffer 1 in two 64-row halves (8 KB per
//      wave instead of 16 KB);
//   3. barrier (buffer 1 free), issues B(1) into it, and waits for A(0) / B(0) with a COUNTED vmcnt
//      that leaves this epilogue's stores (and B(1)) in flight: loads, stores and LDS-DMA retire in
//      issue order, so vmcnt(stores + 4) retires exactly the 8 older pieces;
//   4. re-staggers the wave groups and enters the next tile's main loop (mainloop_bal's body).
// Tiles: workgroup b takes virtual block ids b, b + G, b + 2G, ... (G = grid, a multiple of 8) through
// the same bijective XCD remap + GROUP_M order as gemm_nt_kernel, so the tiles an XCD runs at once
// are the same adjacent ones. Full tiles only (M, N multiples of 256), 16-bit NT, no fp8 codes.
__device__ __forceinline__ void tile_coords(int v, int tiles_m, int tiles_n, int& m0, int& n0, int& tm) {
  panel_coords(xcd_remap(v, tiles_m * tiles_n), tiles_m, tiles_n, m0, n0, tm);
}

// vector-memory instructions one wave's epilogue issues after the next tile's A(0) / B(0) pieces,
// counting only those that can still be in flight at the wait: the stores (its loads are consumed
// inside the epilogue, so they have retired). Must not exceed the true count (a larger vmcnt would
// let A(0) / B(0) through unretired): C 16, + pre-activation or gelu' 16, + the bias-grad partial row
// 2 (lanes 0..7).
template <int EPI, int Q8 = 0> constexpr int epi_stores() {
  return 16 + (epi_gelu_fwd(EPI) ? 16 : 0) + (epi_colsum(EPI) ? 2 : 0) + (Q8 != 0 ? 16 : 0);  // (+ the fp8 codes, 8 B per slot)
}

// fp8 (TI = uint8_t codes, formats FA / FB, dequantised by alpha_a[0] * alpha_b[0]; Q8: the output's
// own fp8 codes too): the same tile walk with mainloop_bk64's body (the fp8 instantiations keep it:
// the balanced loop's extra live fragment spills there) and 128-element K-tiles.
template <typename T, int EPI, typename TI = T, int FA = -1, int FB = -1, int Q8 = 0, int DBG = 0>
__global__ void __launch_bounds__(G_THREADS) gemm_persist_kernel(const TI* __restrict__ A, const TI* __restrict__ B,
                                                                 T* __restrict__ C, int M, int N, int K, int64_t lda,
                                                                 int64_t ldb, int64_t ldc, const T* __restrict__ bias,
                                                                 const T* __restrict__ aux, int64_t ldaux,
                                                                 T* __restrict__ aux_out, float* __restrict__ part,
                                                                 uint64_t* __restrict__ trace,
                                                                 const float* __restrict__ alpha_a = nullptr,
                                                                 const float* __restrict__ alpha_b = nullptr,
                                                                 Q8Out q8 = Q8Out{}) {
  __shared__ __attribute__((aligned(16))) char smem[G_LDS_BYTES];
  __shared__ float q8red[G_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;
  const int tiles_m = M / GB_M, tiles_n = N / GB_N, nwg = tiles_m * tiles_n;
  const int G = gridDim.x;
  constexpr bool F8 = FA >= 0;
  constexpr int BKE = 128 / (int)sizeof(TI);
  const int nt = K / BKE;
  int v = blockIdx.x;
  if (v >= nwg) return;  // (the host sizes the grid to at most the tile count)
  float alpha = 1.f;
  if constexpr (F8) alpha = alpha_a[0] * alpha_b[0];
  if constexpr (Q8 != 0) {  // per-wave running max|C| over the tiles, in LDS (no register across the K loop)
    if (lane == 0) q8red[wid] = 0.f;
  }
  int m0, n0, tm;
  tile_coords(v, tiles_m, tiles_n, m0, n0, tm);
  // first tile's prologue (mainloop_bal's): A(0), B(0) -> buffer 0, B(1) -> buffer 1
  stage_pieces<TI, false>(A, lda, m0, M, 0, smem, wid, lane, 0);
  stage_pieces<TI, false>(A, lda, m0, M, 0, smem, wid, lane, 2);
  stage_pieces<TI, false>(B, ldb, n0, N, 0, smem + G_TILE_BYTES, wid, lane, 0);
  stage_pieces<TI, false>(B, ldb, n0, N, 0, smem + G_TILE_BYTES, wid, lane, 2);
  if (nt > 1) {
    stage_pieces<TI, false>(B, ldb, n0, N, BKE, smem + G_BUF_BYTES + G_TILE_BYTES, wid, lane, 0);
    stage_pieces<TI, false>(B, ldb, n0, N, BKE, smem + G_BUF_BYTES + G_TILE_BYTES, wid, lane, 2);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  bar();
  for (;;) {
    uint64_t tr0 = 0, tr1 = 0;
    if constexpr (DBG & kLabTrace) tr0 = __builtin_amdgcn_s_memrealtime();
    f32x4 acc[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (wr == 1) bar();  // stagger group 1 by one barrier
    // the K loop's per-lane addresses from an opaque lane copy: recomputed per tile rather than kept
    // live through the epilogue (where they spilled, and a scratch reload at the next tile's start
    // waits, in vmcnt order, for every epilogue store still in flight)
    const int lane_k = lane_id_fresh();
    if constexpr (F8) {
      mainloop_bk64_loop<TI, false, FA, FB, 0, true>(A, B, M, N, K, lda, ldb, m0, n0, smem, wid, wr, wc, lane_k, acc);
    } else {
      const int lrk = lane_k & 15, lkk = lane_k >> 4;
      s16x8 fa[4][2], fb[2][2][2];
      read_fb<false>(fb[0], smem + G_TILE_BYTES, wc * 64, lrk, lkk);  // tile 0's first B half
      int t = 0;
      for (; t + 1 < nt; t += 2) {
        bal_tile<TI, false, -1, -1, 0, 0>(t, nt, A, B, M, N, lda, ldb, m0, n0, smem, wid, wr, wc, lane_k, acc, fa, fb);
        bal_tile<TI, false, -1, -1, 0, 1>(t + 1, nt, A, B, M, N, lda, ldb, m0, n0, smem, wid, wr, wc, lane_k, acc, fa,
                                          fb);
      }
      if (t < nt)
        bal_tile<TI, false, -1, -1, 0, 0>(t, nt, A, B, M, N, lda, ldb, m0, n0, smem, wid, wr, wc, lane_k, acc, fa, fb);
    }
    if (wr == 0) bar();  // re-align the groups
    bar();               // every wave is past its last ds_read of this tile
    if constexpr (DBG & kLabTrace) tr1 = __builtin_amdgcn_s_memrealtime();
    const int vn = v + G;
    const bool more = vn < nwg;
    int m1 = 0, n1 = 0, tm1 = 0;
    // an opaque copy of the lane id: everything the epilogue and the next tile's staging derive from
    // it is computed here, not hoisted above the K loop (where it stayed live and spilled ~55 VGPRs)
    const int lane_e = lane_id_fresh();
    if (more) {
      tile_coords(vn, tiles_m, tiles_n, m1, n1, tm1);
    } else {  // the last tile re-loads its own first K-tile (unused): the epilogue's counted waits
      m1 = m0;  // assume exactly 8 pieces behind its first loads
      n1 = n0;
    }
    // the next tile's A(0), B(0): issued by the epilogue after its own first loads (hook)
    auto next_k0 = [&]() {
      stage_pieces<TI, false>(A, lda, m1, M, 0, smem, wid, lane_e, 0);
      stage_pieces<TI, false>(A, lda, m1, M, 0, smem, wid, lane_e, 2);
      stage_pieces<TI, false>(B, ldb, n1, N, 0, smem + G_TILE_BYTES, wid, lane_e, 0);
      stage_pieces<TI, false>(B, ldb, n1, N, 0, smem + G_TILE_BYTES, wid, lane_e, 2);
    };
    __builtin_amdgcn_sched_barrier(0);
    float q8w = 0.f;
    epilogue<T, EPI, false, 0, 4, false, Q8, true, decltype(next_k0), (DBG >> kLabEpiShift) & (kEpiNoMath | kEpiNoStore)>(acc, smem + G_BUF_BYTES + wid * 8192, C, M, N, ldc, bias, aux,
                                                    ldaux, aux_out, part, m0, n0, tm, wr, wc, lane_e, alpha, q8,
                                                    next_k0, &q8w);
    if constexpr (Q8 != 0) {
      const float m = f8_wave_max(q8w);
      if (lane_e == 0) q8red[wid] = fmaxf(q8red[wid], m);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (DBG & kLabTrace) trace_record(trace + (int64_t)v * 4, tr0, tr1, tid);
    if (!more) break;
    bar();  // every wave is done with its epilogue region: buffer 1 is free
    if (nt > 1) {
      stage_pieces<TI, false>(B, ldb, n1, N, BKE, smem + G_BUF_BYTES + G_TILE_BYTES, wid, lane_e, 0);
      stage_pieces<TI, false>(B, ldb, n1, N, BKE, smem + G_BUF_BYTES + G_TILE_BYTES, wid, lane_e, 2);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(((DBG >> kLabEpiShift) & kEpiNoStore ? 0 : epi_stores<EPI, Q8>()) + 4) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DBG >> kLabEpiShift) & kEpiNoStore ? 0 : epi_stores<EPI, Q8>()) : "memory");
    }
    bar();  // A(0), B(0) of the next tile visible to every wave
    v = vn;
    m0 = m1;
    n0 = n1;
    tm = tm1;
  }
  if constexpr (Q8 != 0) {  // one amax atomic per workgroup, after its last tile
    bar();
    if (wid == 0 && lane_id_fresh() == 0) {
      float mm = 0.f;
#pragma unroll
      for (int w = 0; w < G_THREADS / 64; ++w) mm = fmaxf(mm, q8red[w]);
      if (mm > 0.f) f8_atomic_max_pos(q8.amax, mm);
    }
  }
}


// 2-D transpose out[C][R] = in[R][C] (16-bit elements). Each lane transposes an 8x8 block in
// registers: 8 x 16-B row loads, 8 x 16-B row stores. A wave is 8 (along C) x 8 (along R) blocks,
// so every load and every store instruction moves whole 128-B row runs. Edge blocks fall back to
// element-wise accesses.
template <typename T>
__global__ void __launch_bounds__(256) transpose_kernel(const T* __restrict__ in, T* __restrict__ out, int R, int Cc) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int bc = lane & 7, br = lane >> 3;
  // block tile = 64 (C) x 256 (R) per workgroup: 4 waves along R
  const int c0 = blockIdx.x * 64 + bc * 8;
  const int r0 = blockIdx.y * 256 + wid * 64 + br * 8;
  if (c0 + 8 <= Cc && r0 + 8 <= R && (Cc % 8) == 0 && (R % 8) == 0) {
    s16x8 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = *reinterpret_cast<const s16x8*>(in + (int64_t)(r0 + k) * Cc + c0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s16x8 o;
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = v[k][i];
      *reinterpret_cast<s16x8*>(out + (int64_t)(c0 + i) * R + r0) = o;
    }
  } else {
    for (int k = 0; k < 8; ++k)
      for (int i = 0; i < 8; ++i)
        if (r0 + k < R && c0 + i < Cc) out[(int64_t)(c0 + i) * R + r0 + k] = in[(int64_t)(r0 + k) * Cc + c0 + i];
  }
}


}  // namespace
}  // namespace apex
