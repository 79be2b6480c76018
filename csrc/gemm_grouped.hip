// Grouped MFMA GEMMs for mixture-of-experts layers: E independent products whose row counts are
// decided on the device (a router), in one launch each and with no host read of the counts.
//
// Segment layout (apex/ops/grouped.py): activations are one [R, K] tensor of expert-sorted rows and
// `offsets`, int32 [E + 1] on the device: offsets[0] = 0, non-decreasing, every entry a multiple of
// 64, offsets[E] <= R. Expert e owns rows [offsets[e], offsets[e + 1]) (possibly none), the rows that
// pad a segment to its multiple of 64 hold zeros, rows from offsets[E] on are an unused tail.
//
//   gemm_grouped_nt   Y[seg_e, :] = X[seg_e, :] . W[e]^T     W [E, N, K]   forward, and the input
//                                                                          gradient on W^T [E, K, N]
//   gemm_grouped_tt   dW[e] = dY[seg_e]^T . X[seg_e]         dW [E, N, K]  weight gradient, in the
//                     operand dtype (EPI_NONE) or added into an fp32 accumulator (EPI_F32_ACC)
//
// Both are new kernel shells around gemm.hip's device pieces (this unit includes gemm_kernels.h and so
// has its own copies of them): the 256x256x64 ping-pong main loop mainloop_bal — K-contiguous staging
// for NT, transposed-read (TrSrc, ds_read_b64_tr_b16) for TT — and the bounds-checked epilogue.
// Every output element has exactly one writer and there are no atomics: results are bit-reproducible.
//
// gemm_grouped_nt: tile map and order
//  * The M-tile list is virtual: expert e contributes ceil(rows_e / 256) M-tiles, then the tail
//    ceil((R - offsets[E]) / 256). The host cannot know its length, so the grid is the static bound
//    (R / 256 + E + 1) * tiles_n (each of the E + 1 ranges ends in at most one partial tile).
//  * Every workgroup scans the E + 1 offsets itself. The loop index and the pointer are wave-uniform,
//    so the loads are scalar loads of one cached 4 (E + 1)-byte line and the counters live in SGPRs:
//    two passes (total tile count, then the owner of this workgroup's M-tile) cost a few hundred
//    scalar instructions next to a 256x256xK tile. The alternative, a table-building pre-kernel, adds
//    a launch and a device buffer to every GEMM of every layer for nothing the scan cannot do.
//  * Workgroups at or past the real tile count return before any barrier. The XCD remap runs over the
//    REAL count: the surplus workgroups are the highest block ids, dealt round-robin like all others,
//    so every XCD keeps an equal share of real tiles (a remap over the grid bound would leave the
//    last XCD's contiguous range mostly empty).
//  * Order: bijective XCD remap, then gemm.hip's GROUP_M panel order over (virtual M-tile, N-tile): 8
//    consecutive M-tiles down one N column before moving right. Consecutive virtual M-tiles are
//    consecutive row blocks of one expert (and then of the next), so the workgroups an XCD runs at
//    once read ONE 256-row panel of one W[e] (two where a segment ends) and adjacent X panels out of
//    its L2, exactly the sharing the dense kernel's order is built for.
//  * Per tile A = X + offsets[e] lda, M = rows_e, B = W + e N K, C = Y + offsets[e] ldc: the staging's
//    row clamp and the epilogue's bounds check then stay inside the expert's own segment. Segments
//    end on multiples of 64, not 256, so partial tiles are the common case and the kernel has the
//    bounds-checked epilogue only (one epilogue variant per kernel, as gemm_epilogue.h asks).
//  * Tail tiles store zeros: Y comes from an uninitialised allocation and feeds elementwise kernels.
//
// gemm_grouped_tt: grid (tiles(N, K), E), blockIdx.y = expert, no split-K (tiles * E exceeds the CU count at MoE
// shapes; an assumption from shapes, see profiles/README.md). Inside an expert the tiles take gemm.hip's order
// (XCD remap over the expert's tiles, then GROUP_M panels), so every expert's tiles are spread over all
// eight XCDs: the experts' contraction lengths differ, and an order that gives an XCD one expert's tiles
// (measured: with a joint expert-major remap the E = 8 weight gradient took 2853 us with one expert holding half of
// 16384 rows against 961 us balanced; with this order 966 and 960 us, profiles/grouped_gemm_vs_loop.jsonl) leaves
// seven XCDs idle behind the longest expert. An empty expert never enters the main loop (its prologue
// would stage K-tile 0 unconditionally): the branch on the wave-uniform row count comes before the first
// load; EPI_NONE stores zeros, EPI_F32_ACC returns.
#include "gemm_kernels.h"

namespace apex {
namespace {

// zeros into rows [m0, m0 + 256) x cols [n0, n0 + 256) of C [M, N] (N % 8 == 0), 16 bytes per store
template <typename T>
__device__ __forceinline__ void zero_tile(T* __restrict__ C, int M, int N, int64_t ldc, int m0, int n0, int tid) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll 4
  for (int i = tid; i < GB_M * (GB_N / 8); i += G_THREADS) {
    const int m = m0 + i / (GB_N / 8), n = n0 + (i % (GB_N / 8)) * 8;
    if (m < M && n < N) *reinterpret_cast<u32x4*>(C + (int64_t)m * ldc + n) = u32x4{0u, 0u, 0u, 0u};
  }
}

__device__ __forceinline__ int tiles_of(int rows) { return (rows + GB_M - 1) / GB_M; }

// Range e of the table (e < E: expert e, e == E: the tail) as (first row, row count), wave-uniform. The
// entries are clamped to [0, R] and to multiples of 64, so that a table that breaks the layout's contract
// yields wrong numbers, never an address outside the tensors or a misaligned 16-byte access.
__device__ __forceinline__ void seg_range(const int* __restrict__ offsets, int e, int E, int R, int& row0, int& rows) {
  row0 = min(max(offsets[e], 0), R) & ~(GB_K - 1);
  const int end = e < E ? min(max(offsets[e + 1], 0), R) & ~(GB_K - 1) : R;
  rows = max(end - row0, 0);
}

template <typename T>
__global__ void __launch_bounds__(G_THREADS) gemm_grouped_nt_kernel(const T* __restrict__ X, const T* __restrict__ W,
                                                                    T* __restrict__ Y, const int* __restrict__ offsets,
                                                                    int E, int R, int N, int K, int64_t lda, int64_t ldc) {
  __shared__ __attribute__((aligned(16))) char smem[G_LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;

  // ---- pass 1: the real length of the virtual M-tile list (ranges 0..E-1: experts, E: the tail) ----
  const int tiles_n = (N + GB_N - 1) / GB_N;
  int tiles_m = 0;
  for (int e = 0; e <= E; ++e) {
    int row0, rows;
    seg_range(offsets, e, E, R, row0, rows);
    tiles_m += tiles_of(rows);
  }
  const int nwg = tiles_m * tiles_n;
  const int bid = blockIdx.x;
  if (bid >= nwg) return;  // surplus of the static grid bound: before any barrier
  int m0, n0, tm;
  panel_coords(xcd_remap(bid, nwg), tiles_m, tiles_n, m0, n0, tm);
  // ---- pass 2: the range that owns virtual M-tile tm, and the tile's index inside it ----
  int e = 0, row0 = 0, rows = 0;
  for (int t = tm;; ++e) {
    seg_range(offsets, e, E, R, row0, rows);
    const int n = tiles_of(rows);
    if (t < n) {
      m0 = t * GB_M;
      break;
    }
    t -= n;
  }
  T* C = Y + (int64_t)row0 * ldc;
  if (e == E) {
    zero_tile<T>(C, rows, N, ldc, m0, n0, tid);
    return;
  }
  const T* A = X + (int64_t)row0 * lda;
  const T* B = W + (int64_t)e * N * K;

  f32x4 acc[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  mainloop_bal<T, false>(A, B, rows, N, K, lda, (int64_t)K, m0, n0, smem, wid, wr, wc, lane, acc);
  if (wr == 0) bar();  // re-align the groups
  bar();               // every wave is past its last ds_read: LDS is free for the epilogue
  epilogue<T, EPI_NONE, true>(acc, smem + wid * 16384, C, rows, N, ldc, (const T*)nullptr, (const T*)nullptr,
                              (int64_t)0, (T*)nullptr, (float*)nullptr, m0, n0, tm, wr, wc, lane);
}

// dW[e] [P, Q] (+)= A[seg_e]^T B[seg_e], A = dY [R, P], B = X [R, Q]; blockIdx.y = expert
template <typename T, int EPI, bool EDGE>
__global__ void __launch_bounds__(G_THREADS) gemm_grouped_tt_kernel(const T* __restrict__ A, const T* __restrict__ B,
                                                                    T* __restrict__ C, float* __restrict__ part,
                                                                    const int* __restrict__ offsets, int R, int P, int Q) {
  static_assert(EPI == EPI_NONE || EPI == EPI_F32_ACC, "grouped weight gradient: dW in T, or += into fp32");
  __shared__ __attribute__((aligned(16))) char smem[G_LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;
  const int lr = lane & 15, lk = lane >> 4;

  const int tiles_m = (P + GB_M - 1) / GB_M, tiles_n = (Q + GB_N - 1) / GB_N;
  const int nwg = tiles_m * tiles_n;
  const int e = blockIdx.y;
  int m0, n0, tm;
  panel_coords(xcd_remap((int)blockIdx.x, nwg), tiles_m, tiles_n, m0, n0, tm);

  int row0, rows;
  seg_range(offsets, e, (int)gridDim.y, R, row0, rows);  // whole K-tiles (the layout's contract)
  const int64_t slab = (int64_t)e * P * Q;
  if (rows == 0) {  // empty expert: wave-uniform, before the first load
    if constexpr (EPI == EPI_NONE) zero_tile<T>(C + slab, P, Q, (int64_t)Q, m0, n0, tid);
    return;
  }

  f32x4 acc[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  mainloop_bal<T, true>(A + (int64_t)row0 * P, B + (int64_t)row0 * Q, P, Q, rows, (int64_t)P, (int64_t)Q, m0, n0, smem,
                        wid, wr, wc, lane, acc);
  if (wr == 0) bar();
  bar();
  if constexpr (EPI == EPI_F32_ACC) {
    // out[m, n] += acc in fp32, in two halves of 16 fragments whose 16-byte loads are all issued before
    // the first add (gemm_nt_kernel's read-modify-write epilogue)
    float* out = part + slab;
    const int64_t ldc = Q;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      f32x4 prev[2][8];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int n = n0 + wc * 64 + (2 * hf + jj) * 16 + 4 * lk;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int m = m0 + wr * 128 + i * 16 + lr;
          prev[jj][i] = m < P && n < Q ? *reinterpret_cast<const f32x4*>(out + (int64_t)m * ldc + n) : f32x4{};
        }
      }
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int n = n0 + wc * 64 + (2 * hf + jj) * 16 + 4 * lk;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int m = m0 + wr * 128 + i * 16 + lr;
          if (m < P && n < Q) *reinterpret_cast<f32x4*>(out + (int64_t)m * ldc + n) = prev[jj][i] + acc[2 * hf + jj][i];
        }
      }
    }
  } else {
    epilogue<T, EPI_NONE, EDGE>(acc, smem + wid * 16384, C + slab, P, Q, (int64_t)Q, (const T*)nullptr,
                                (const T*)nullptr, (int64_t)0, (T*)nullptr, (float*)nullptr, m0, n0, tm, wr, wc, lane);
  }
}

template <typename T>
void launch_grouped_nt(const GroupedGemmArgs& g, hipStream_t s) {
  const int tiles_n = (g.N + GB_N - 1) / GB_N;
  const int grid = (g.R / GB_M + g.E + 1) * tiles_n;
  hipLaunchKernelGGL((gemm_grouped_nt_kernel<T>), dim3(grid), dim3(G_THREADS), 0, s, (const T*)g.A, (const T*)g.B,
                     (T*)g.C, g.offsets, g.E, g.R, g.N, g.K, (int64_t)g.K, (int64_t)g.N);
}

template <typename T, int EPI>
void launch_grouped_tt(const GroupedGemmArgs& g, hipStream_t s) {
  // P = g.N (dY's columns), Q = g.K (X's columns)
  const int tiles = ((g.N + GB_M - 1) / GB_M) * ((g.K + GB_N - 1) / GB_N);
  if (g.N % GB_M != 0 || g.K % GB_N != 0)
    hipLaunchKernelGGL((gemm_grouped_tt_kernel<T, EPI, true>), dim3(tiles, g.E), dim3(G_THREADS), 0, s, (const T*)g.A,
                       (const T*)g.B, (T*)g.C, g.acc, g.offsets, g.R, g.N, g.K);
  else
    hipLaunchKernelGGL((gemm_grouped_tt_kernel<T, EPI, false>), dim3(tiles, g.E), dim3(G_THREADS), 0, s, (const T*)g.A,
                       (const T*)g.B, (T*)g.C, g.acc, g.offsets, g.R, g.N, g.K);
}

}  // namespace

bool gemm_grouped_supported(int64_t R, int64_t K, int64_t N, int64_t E) {
  // N < 2^22: the epilogue addresses a 128-row wave tile through 32-bit buffer offsets (ldc = N; the weight
  // gradient's ldc = K, and its TrSrc offsets need ld < 2^28); R K < 2^40 as gemm_supported
  const int64_t tiles_n = (N + GB_N - 1) / GB_N;
  return R > 0 && K > 0 && N > 0 && E >= 1 && K % GB_K == 0 && N % 8 == 0 && R % 64 == 0 && N < (1 << 22) &&
         K < (1 << 22) && R < (1ll << 31) && R * K < (1ll << 40) && E < (1 << 16) &&
         (R / GB_M + E + 1) * tiles_n < (1ll << 31) && tiles_n * ((K + GB_N - 1) / GB_N) * E < (1ll << 31);
}

int gemm_grouped_nt(const GroupedGemmArgs& g, int dt, hipStream_t s) {
  if (!gemm_grouped_supported(g.R, g.K, g.N, g.E) || !g.offsets) return -2;
  if (dt == kBF16Code) launch_grouped_nt<bf16>(g, s);
  else if (dt == kF16Code) launch_grouped_nt<f16>(g, s);
  else return -1;
  return (int)hipGetLastError();
}

int gemm_grouped_tt(const GroupedGemmArgs& g, int dt, hipStream_t s) {
  if (!gemm_grouped_supported(g.R, g.K, g.N, g.E) || !g.offsets) return -2;
  if ((g.acc != nullptr) == (g.C != nullptr)) return -3;  // exactly one output
  if (dt == kBF16Code) {
    if (g.acc) launch_grouped_tt<bf16, EPI_F32_ACC>(g, s);
    else launch_grouped_tt<bf16, EPI_NONE>(g, s);
  } else if (dt == kF16Code) {
    if (g.acc) launch_grouped_tt<f16, EPI_F32_ACC>(g, s);
    else launch_grouped_tt<f16, EPI_NONE>(g, s);
  } else {
    return -1;
  }
  return (int)hipGetLastError();
}

}  // namespace apex
