// Hand-written MFMA GEMM for gfx950 with fused epilogues (the transformer dense layers).
//
//   C[M,N] = epilogue( A[M,K] . B[N,K]^T )      A, B, C row-major, bf16 or fp16, fp32 accumulate
//
// Both operands are K-contiguous ("NT"): the forward projections (X . W^T) directly, and the
// input-gradient GEMMs (dY . W) through a transposed copy of W (transpose_2d below).
// Weight gradients (contraction over tokens): the transposed-read instantiation (gemm_tt, split-K
// fp32 slabs) for the shapes where it beats hipBLASLt, the library split-K otherwise (fused.py).
//
// Epilogues (fused into the tile write, so the activation never makes an extra HBM round
// trip — the separate bias/GELU/residual kernels they replace each read+wrote [M,N]):
//   EPI_NONE      C = acc
//   EPI_BIAS      C = acc + bias[n]
//   EPI_BIAS_GELU H = acc + bias[n] (pre-activation, kept for backward), C = gelu(H)
//   EPI_DGELU     C = acc * gelu'(H[m,n])   and per-(256-row tile, wave row) column partial sums
//                 of C written to `part` (the bias gradient, finished by partial_colsum)
//   EPI_RESID     C = acc + R[m,n]          (residual-gradient accumulation)
//   EPI_BIAS_GELU_TANH / EPI_DGELU_TANH: the same with the tanh-approximated GELU (GPT-2)
//   EPI_BIAS_GELU_D / _TANH_D  C = gelu(H) and gelu'(H) stored instead of H: the derivative shares
//                 the exp / erf (or sigmoid) of the GELU, so it is a few FMAs here, and the backward
//                 epilogue becomes
//   EPI_MUL       C = acc * G[m,n] with the bias-gradient partials of EPI_DGELU — a multiply
//                 instead of the erf/exp evaluation that made the dGELU epilogue VALU-bound
//                 (404 vs 201 us main loop at M=32768 N=4096 K=1024, profiles/r1_gemm_stagger.json)
//
// Tiling (CDNA4, cdna_hip_programming.md §5):
//  * 256x256 output tile, BK = 64, 512 threads = 8 waves as 2 (M) x 4 (N); each wave owns a
//    128 x 64 sub-tile = 8 x 4 fragments of v_mfma_f32_16x16x32 (128 fp32 accumulators/lane).
//  * The MFMA is issued "swapped" (A-operand = B rows, B-operand = A rows) so each lane ends
//    with 4 consecutive N-columns of one M-row: 8-byte vector epilogue loads/stores.
//  * Global -> LDS by global_load_lds_dwordx4 (16 B per lane, no VGPR round trip), double
//    buffered (2 x 64 KB), the next K-tile in flight across the barrier (counted vmcnt, raw
//    s_barrier — never __syncthreads(), whose fence would drain the prefetch).
//  * LDS image: 128-byte rows (64 bf16 of K), 16-byte chunk c of row r stored at chunk
//    c ^ ((r >> 1) & 7). glds writes lane-linear, so the XOR is applied to the per-lane SOURCE
//    address and again on the ds_read_b128: every 16-lane ds_read_b128 group then touches 16
//    distinct 16-B slots of the 256-B bank row (conflict-free).
//  * blockIdx -> tile: bijective XCD remap (each XCD gets a contiguous tile range) then
//    GROUP_M=8 panel ordering, so concurrently running tiles on one XCD share A/B panels in L2.
//
// This file: the launchers, the *_supported predicates and the exported API. The device code is in
// gemm_mainloop.h (staging, fragments, K loops), gemm_epilogue.h and gemm_kernels.h.
#include "gemm_kernels.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace apex {
namespace {

// An on / off environment flag: unset -> dflt; set, a default-on flag is turned off by "0..." and a
// default-off one turned on by "1..."; callers keep the value in a function-local static (read once)
inline bool env_flag(const char* name, bool dflt) {
  const char* e = getenv(name);
  return e ? (dflt ? e[0] != '0' : e[0] == '1') : dflt;
}

int h_gemm_dbg = 0, h_gemm_stagger = 0;  // gemm_set_dbg(); stagger: > 0 forced units, < 0 forced off, 0 launcher's
// ctl bit kCtlSplitXcd of the split-K (transposed-read) launches: APEX_GEMM_SPLIT_XCD=0 turns it off (A/B)
inline bool host_split_xcd() {
  static const bool on = env_flag("APEX_GEMM_SPLIT_XCD", true);
  return on;
}

// per-epilogue first-round stagger units from APEX_GEMM_STAGGER="epi:units,..." (experiment; read once)
inline int host_stagger(int epi) {
  static int table[16] = {-1};
  if (table[0] == -1) {
    for (int& t : table) t = 0;
    if (const char* e = getenv("APEX_GEMM_STAGGER")) {
      int ep = 0, u = 0;
      const char* p = e;
      while (*p) {
        if (sscanf(p, "%d:%d", &ep, &u) == 2 && ep >= 0 && ep < 16) table[ep] = u;
        while (*p && *p != ',') ++p;
        if (*p == ',') ++p;
      }
    }
  }
  return table[epi];
}

// Persistent kernel (gemm_persist_kernel) for full-tile 16-bit NT launches: APEX_GEMM_PERSIST=0 turns it
// off (A/B). Measured against the one-tile-per-workgroup kernel at the BERT shapes, same process,
// interleaved, bit-identical outputs (profiles/r5_gemm_persist_m98304.jsonl): 0.7-3.6 % faster on
// every shape (plain / bias 3.6 %, residual 1-3 %, GELU_D 1.9 %, multiply 0.7 %).
// h_gemm_persist / h_gemm_persist_f8: -1 = the environment's choice (read once), 0 / 1 forced by
// gemm_set_persist() (the tests compare both kernels bitwise in one process)
int h_gemm_persist = -1, h_gemm_persist_f8 = -1;
inline bool host_persist() {
  static const bool on = env_flag("APEX_GEMM_PERSIST", true);
  return h_gemm_persist >= 0 ? h_gemm_persist == 1 : on;
}
inline int host_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cus = n;
  }
  return cus;
}

// The persistent kernels' launches: full tiles, more of them than CUs; one workgroup per CU walks them
// (the grid stays a multiple of 8: the XCD remap deals workgroups round-robin)
inline bool persist_shape(const GemmArgs& g) {
  return g.M % GB_M == 0 && g.N % GB_N == 0 && (g.M / GB_M) * (g.N / GB_N) > host_cus();
}
inline dim3 persist_grid() { return dim3((host_cus() / 8) * 8); }

template <typename T, int EPI, bool TR = false>
void launch_gemm(const GemmArgs& g, hipStream_t s) {
  const int tiles = ((g.M + GB_M - 1) / GB_M) * ((g.N + GB_N - 1) / GB_N);
  if constexpr (!TR && EPI != EPI_F32 && EPI != EPI_F32_ACC) {
    if (persist_shape(g) && host_persist() && h_gemm_dbg == 0 && h_gemm_stagger <= 0) {
      hipLaunchKernelGGL((gemm_persist_kernel<T, EPI>), persist_grid(), dim3(G_THREADS), 0, s, (const T*)g.A, (const T*)g.B,
                         (T*)g.C, g.M, g.N, g.K, g.lda, g.ldb, g.ldc, (const T*)g.bias, (const T*)g.aux, g.ldaux,
                         (T*)g.aux_out, g.part, (uint64_t*)nullptr);
      return;
    }
  }
  const int units = h_gemm_stagger > 0 ? h_gemm_stagger : h_gemm_stagger < 0 ? 0 : host_stagger(EPI);
  const int stagger = (units & 0x7fff) | (TR && host_split_xcd() ? kCtlSplitXcd : 0) |
                      (h_gemm_dbg << 16);  // the kernel's ctl word
  const bool edge = g.M % GB_M != 0 || g.N % GB_N != 0;
  if (edge)  // (the transposed-read weight-gradient kernels too: partial tiles since round 5)
    hipLaunchKernelGGL((gemm_nt_kernel<T, EPI, TR, true>), dim3(tiles, TR ? g.splits : 1), dim3(G_THREADS), 0, s,
                       (const T*)g.A, (const T*)g.B, (T*)g.C, g.M, g.N, g.K, g.lda, g.ldb, g.ldc, (const T*)g.bias,
                       (const T*)g.aux, g.ldaux, (T*)g.aux_out, g.part, stagger);
  else
    hipLaunchKernelGGL((gemm_nt_kernel<T, EPI, TR, false>), dim3(tiles, TR ? g.splits : 1), dim3(G_THREADS), 0, s,
                       (const T*)g.A, (const T*)g.B, (T*)g.C, g.M, g.N, g.K, g.lda, g.ldb, g.ldc, (const T*)g.bias,
                       (const T*)g.aux, g.ldaux, (T*)g.aux_out, g.part, stagger);
}

// fp8 launches on the persistent kernel: OFF by default (APEX_GEMM_PERSIST_F8=1 turns it on). Measured
// at the BERT fp8 shapes, M = 98304 (tools/fp8_persist_bench.py, same box, bit-identical outputs):
// first SLOWER on every shape (profiles/r5_fp8_persist_ab.jsonl: FFN2 forward 487 vs 418 us, FFN1
// dgrad + residual 635 vs 438) — the fp8 main loop runs at the 256-VGPR limit, and in the persistent
// kernel a spilled staging address was reloaded inside the K loop behind the previous tile's epilogue
// stores (loads, stores and scratch retire in vmcnt order). With the staging addresses recomputed from
// a fresh lane id per K-tile (FRESH, 0 scratch): still 2-5 % slower except the out-projection forward,
// fp8 BERT step 156.2 vs 155.2 ms (profiles/r5_fp8_persist_ab_v2.jsonl).
inline bool host_persist_f8() {
  static const bool on = env_flag("APEX_GEMM_PERSIST_F8", false);
  return (h_gemm_persist_f8 >= 0 ? h_gemm_persist_f8 == 1 : on) && host_persist();
}

template <typename T, int EPI, int FA, int FB>
void launch_gemm_f8(const GemmArgs& g, hipStream_t s) {
  const int tiles = ((g.M + GB_M - 1) / GB_M) * ((g.N + GB_N - 1) / GB_N);
  // fp8 codes of C for the next GEMM (the MLP's hidden activation forward, its gradient backward)
  constexpr bool Q8_OK = epi_codes_ok(EPI);
  if (persist_shape(g) && host_persist_f8()) {
    auto go = [&](auto q_c) {
      hipLaunchKernelGGL((gemm_persist_kernel<T, EPI, uint8_t, FA, FB, decltype(q_c)::value>), persist_grid(),
                         dim3(G_THREADS), 0, s, (const uint8_t*)g.A, (const uint8_t*)g.B, (T*)g.C, g.M, g.N, g.K, g.lda,
                         g.ldb, g.ldc, (const T*)g.bias, (const T*)g.aux, g.ldaux, (T*)g.aux_out, g.part,
                         (uint64_t*)nullptr, g.alpha_a, g.alpha_b, g.q8);
    };
    if constexpr (Q8_OK) {
      if (g.q8.y) {
        if (g.q8.fmt == 0) go(std::integral_constant<int, 1>{});
        else go(std::integral_constant<int, 2>{});
        return;
      }
    }
    go(std::integral_constant<int, 0>{});
    return;
  }
  // codes-only C (Q8Out::only): the bias+GELU+derivative forward and the multiply backward on full
  // tiles; elsewhere the flag is ignored (C written as well: a superset, never wrong)
  constexpr bool NOC_OK = epi_codes_only_ok(EPI);
  if constexpr (Q8_OK) {
    if (g.q8.y) {
      auto go = [&](auto edge_c, auto q_c, auto noc_c) {
        hipLaunchKernelGGL((gemm_nt_kernel<T, EPI, false, decltype(edge_c)::value, uint8_t, FA, FB, 0,
                                           decltype(q_c)::value, decltype(noc_c)::value>),
                           dim3(tiles), dim3(G_THREADS), 0, s, (const uint8_t*)g.A, (const uint8_t*)g.B, (T*)g.C, g.M,
                           g.N, g.K, g.lda, g.ldb, g.ldc, (const T*)g.bias, (const T*)g.aux, g.ldaux, (T*)g.aux_out,
                           g.part, 0, g.alpha_a, g.alpha_b, g.q8);
      };
      const bool edge = g.M % GB_M != 0 || g.N % GB_N != 0;
      if constexpr (NOC_OK) {
        if (g.q8.only && !edge) {
          if (g.q8.fmt == 0) go(std::false_type{}, std::integral_constant<int, 1>{}, std::true_type{});
          else go(std::false_type{}, std::integral_constant<int, 2>{}, std::true_type{});
          return;
        }
      }
      if (g.q8.fmt == 0) {
        if (edge) go(std::true_type{}, std::integral_constant<int, 1>{}, std::false_type{});
        else go(std::false_type{}, std::integral_constant<int, 1>{}, std::false_type{});
      } else {
        if (edge) go(std::true_type{}, std::integral_constant<int, 2>{}, std::false_type{});
        else go(std::false_type{}, std::integral_constant<int, 2>{}, std::false_type{});
      }
      return;
    }
  }
  if (g.M % GB_M != 0 || g.N % GB_N != 0)
    hipLaunchKernelGGL((gemm_nt_kernel<T, EPI, false, true, uint8_t, FA, FB>), dim3(tiles), dim3(G_THREADS), 0, s,
                       (const uint8_t*)g.A, (const uint8_t*)g.B, (T*)g.C, g.M, g.N, g.K, g.lda, g.ldb, g.ldc,
                       (const T*)g.bias, (const T*)g.aux, g.ldaux, (T*)g.aux_out, g.part, 0, g.alpha_a, g.alpha_b);
  else
    hipLaunchKernelGGL((gemm_nt_kernel<T, EPI, false, false, uint8_t, FA, FB>), dim3(tiles), dim3(G_THREADS), 0, s,
                       (const uint8_t*)g.A, (const uint8_t*)g.B, (T*)g.C, g.M, g.N, g.K, g.lda, g.ldb, g.ldc,
                       (const T*)g.bias, (const T*)g.aux, g.ldaux, (T*)g.aux_out, g.part, 0, g.alpha_a, g.alpha_b);
}

template <typename T, int FA, int FB>
int gemm_dispatch_f8(const GemmArgs& g, hipStream_t s) {
  switch (g.epi) {
    case EPI_NONE: launch_gemm_f8<T, EPI_NONE, FA, FB>(g, s); break;
    case EPI_BIAS: launch_gemm_f8<T, EPI_BIAS, FA, FB>(g, s); break;
    case EPI_RESID: launch_gemm_f8<T, EPI_RESID, FA, FB>(g, s); break;
    case EPI_BIAS_GELU: launch_gemm_f8<T, EPI_BIAS_GELU, FA, FB>(g, s); break;
    case EPI_BIAS_GELU_TANH: launch_gemm_f8<T, EPI_BIAS_GELU_TANH, FA, FB>(g, s); break;
    case EPI_DGELU: launch_gemm_f8<T, EPI_DGELU, FA, FB>(g, s); break;
    case EPI_DGELU_TANH: launch_gemm_f8<T, EPI_DGELU_TANH, FA, FB>(g, s); break;
    case EPI_BIAS_GELU_D: launch_gemm_f8<T, EPI_BIAS_GELU_D, FA, FB>(g, s); break;
    case EPI_BIAS_GELU_TANH_D: launch_gemm_f8<T, EPI_BIAS_GELU_TANH_D, FA, FB>(g, s); break;
    case EPI_MUL: launch_gemm_f8<T, EPI_MUL, FA, FB>(g, s); break;
    default: return -3;
  }
  return (int)hipGetLastError();
}

template <typename T>
int gemm_dispatch(const GemmArgs& g, hipStream_t s) {
  switch (g.epi) {
    case EPI_NONE: launch_gemm<T, EPI_NONE>(g, s); break;
    case EPI_BIAS: launch_gemm<T, EPI_BIAS>(g, s); break;
    case EPI_BIAS_GELU: launch_gemm<T, EPI_BIAS_GELU>(g, s); break;
    case EPI_DGELU: launch_gemm<T, EPI_DGELU>(g, s); break;
    case EPI_BIAS_GELU_TANH: launch_gemm<T, EPI_BIAS_GELU_TANH>(g, s); break;
    case EPI_DGELU_TANH: launch_gemm<T, EPI_DGELU_TANH>(g, s); break;
    case EPI_RESID: launch_gemm<T, EPI_RESID>(g, s); break;
    case EPI_BIAS_GELU_D: launch_gemm<T, EPI_BIAS_GELU_D>(g, s); break;
    case EPI_BIAS_GELU_TANH_D: launch_gemm<T, EPI_BIAS_GELU_TANH_D>(g, s); break;
    case EPI_MUL: launch_gemm<T, EPI_MUL>(g, s); break;
    default: return -3;
  }
  return (int)hipGetLastError();
}

}  // namespace

bool gemm_supported(int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc) {
  // ldc < 2^22: the epilogue addresses a 128-row wave tile through 32-bit buffer offsets
  return M > 0 && N > 0 && K > 0 && K % GB_K == 0 && N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0 &&
         ldc < (1 << 22) &&
         (int64_t)M * lda < (1ll << 40);
}

int64_t gemm_part_rows(int M) { return (int64_t)((M + GB_M - 1) / GB_M) * 2; }

int gemm_set_dbg(int v) {
  // v < 0: -v = stagger units (experiment); v >= 0: diagnostics mode
  if (v < 0) {  // -100: force no stagger; -200: launcher's choice; -k: k units
    h_gemm_stagger = v == -100 ? -1 : v == -200 ? 0 : -v;
    return 0;
  }
  h_gemm_dbg = v;
  return 0;
}

// which = 0: the 16-bit persistent kernel, 1: the fp8 one; v = 1 on, 0 off, -1 back to the environment's
// choice. Returns the previous forced value.
int gemm_set_persist(int which, int v) {
  int& h = which == 1 ? h_gemm_persist_f8 : h_gemm_persist;
  const int prev = h;
  h = v < 0 ? -1 : (v ? 1 : 0);
  return prev;
}

int gemm_nt(const GemmArgs& g, int dt, hipStream_t s) {
  if (!gemm_supported(g.M, g.N, g.K, g.lda, g.ldb, g.ldc)) return -2;
  if (g.aux && g.ldaux >= (1 << 22)) return -2;  // 32-bit buffer offsets in the epilogue
  if (dt == kBF16Code) return gemm_dispatch<bf16>(g, s);
  if (dt == kF16Code) return gemm_dispatch<f16>(g, s);
  return -1;
}

bool gemm_f8_supported(int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc) {
  return M > 0 && N > 0 && K > 0 && K % 128 == 0 && N % 8 == 0 && lda % 16 == 0 && ldb % 16 == 0 && ldc % 8 == 0 &&
         ldc < (1 << 22) &&
         (int64_t)M * lda < (1ll << 40);
}

int gemm_nt_f8(const GemmArgs& g, int fmt_a, int fmt_b, int out_dt, hipStream_t s) {
  // A (activations / gradients): e4m3 (0) or e5m2 (1); B (weights): e4m3
  if (!gemm_f8_supported(g.M, g.N, g.K, g.lda, g.ldb, g.ldc) || fmt_b != 0 || !g.alpha_a || !g.alpha_b) return -2;
  if (g.aux && g.ldaux >= (1 << 22)) return -2;
  if (out_dt == kBF16Code) {
    if (fmt_a == 0) return gemm_dispatch_f8<bf16, 0, 0>(g, s);
    if (fmt_a == 1) return gemm_dispatch_f8<bf16, 1, 0>(g, s);
  } else if (out_dt == kF16Code) {
    if (fmt_a == 0) return gemm_dispatch_f8<f16, 0, 0>(g, s);
    if (fmt_a == 1) return gemm_dispatch_f8<f16, 1, 0>(g, s);
  }
  return -1;
}

bool gemm_tt_supported(int P, int Q, int R, int splits, int64_t lda, int64_t ldb) {
  // P, Q: any multiple of 8 (partial 256-tiles: clamped staging + bounds-checked epilogues);
  // ld < 2^28: TrSrc's 32-bit per-lane offsets span the 8 K-rows a wave stages
  return P > 0 && Q > 0 && splits > 0 && P % 8 == 0 && Q % 8 == 0 && R % GB_K == 0 && R / GB_K >= splits &&
         lda % 8 == 0 && ldb % 8 == 0 && lda >= P && ldb >= Q && lda < (1 << 28) && ldb < (1 << 28);
}

int gemm_tt(const GemmArgs& g, int dt, hipStream_t s) {
  // C[P=M, Q=N] (+)= sum_r A[r, p] B[r, q]; g.K = ALL contraction rows (g.splits slices of whole K-tiles,
  // sizes within one K-tile of each other); g.part = fp32 slabs
  // [splits, M, N] when g.epi == EPI_F32, the fp32 [M, N] accumulator (+=) when EPI_F32_ACC, else g.C
  // in the operand dtype (splits must be 1 except for EPI_F32)
  if (!gemm_tt_supported(g.M, g.N, g.K, g.splits, g.lda, g.ldb)) return -2;
  if (g.epi != EPI_F32 && ((g.epi != EPI_NONE && g.epi != EPI_F32_ACC) || g.splits != 1)) return -3;
  if (dt == kBF16Code) {
    if (g.epi == EPI_F32) launch_gemm<bf16, EPI_F32, true>(g, s);
    else if (g.epi == EPI_F32_ACC) launch_gemm<bf16, EPI_F32_ACC, true>(g, s);
    else launch_gemm<bf16, EPI_NONE, true>(g, s);
  } else if (dt == kF16Code) {
    if (g.epi == EPI_F32) launch_gemm<f16, EPI_F32, true>(g, s);
    else if (g.epi == EPI_F32_ACC) launch_gemm<f16, EPI_F32_ACC, true>(g, s);
    else launch_gemm<f16, EPI_NONE, true>(g, s);
  } else {
    return -1;
  }
  return (int)hipGetLastError();
}

bool gemm_tt_f8_supported(int P, int Q, int R, int splits, int64_t lda, int64_t ldb) {
  // fp8 codes: 16-byte chunks of 16 columns (partial 256-tiles clamp to the last full chunk);
  // ld < 2^28: TrSrc's 32-bit per-lane offsets span the 16 K-rows a wave stages
  return P > 0 && Q > 0 && splits > 0 && P % 16 == 0 && Q % 16 == 0 && R % 128 == 0 && R / 128 >= splits &&
         lda % 16 == 0 && ldb % 16 == 0 && lda >= P && ldb >= Q && lda < (1 << 28) && ldb < (1 << 28);
}

// fp8 weight gradient: fp32 slabs [splits, P, Q] of alpha_a alpha_b sum_r A[r, p] B[r, q] over the
// uint8 codes A (format fmt_a: the output gradient, e5m2 in the hybrid recipe) and B (fmt_b: the
// layer input, e4m3); the transposed-read main loop with ds_read_b64_tr_b8 fragments
template <int FA, int FB>
void launch_gemm_tt_f8(const GemmArgs& g, hipStream_t s) {
  const int tiles = ((g.M + GB_M - 1) / GB_M) * ((g.N + GB_N - 1) / GB_N);
  if (g.M % GB_M != 0 || g.N % GB_N != 0)
    hipLaunchKernelGGL((gemm_nt_kernel<bf16, EPI_F32, true, true, uint8_t, FA, FB>), dim3(tiles, g.splits),
                       dim3(G_THREADS), 0, s, (const uint8_t*)g.A, (const uint8_t*)g.B, (bf16*)nullptr, g.M, g.N, g.K,
                       g.lda, g.ldb, g.ldc, (const bf16*)nullptr, (const bf16*)nullptr, (int64_t)0, (bf16*)nullptr,
                       g.part, host_split_xcd() ? kCtlSplitXcd : 0, g.alpha_a, g.alpha_b);
  else
    hipLaunchKernelGGL((gemm_nt_kernel<bf16, EPI_F32, true, false, uint8_t, FA, FB>), dim3(tiles, g.splits),
                       dim3(G_THREADS), 0, s, (const uint8_t*)g.A, (const uint8_t*)g.B, (bf16*)nullptr, g.M, g.N, g.K,
                       g.lda, g.ldb, g.ldc, (const bf16*)nullptr, (const bf16*)nullptr, (int64_t)0, (bf16*)nullptr,
                       g.part, host_split_xcd() ? kCtlSplitXcd : 0, g.alpha_a, g.alpha_b);
}

int gemm_tt_f8(const GemmArgs& g, int fmt_a, int fmt_b, hipStream_t s) {
  if (!gemm_tt_f8_supported(g.M, g.N, g.K, g.splits, g.lda, g.ldb) || !g.alpha_a || !g.alpha_b ||
      !g.part)
    return -2;
  if (fmt_a == 1 && fmt_b == 0) launch_gemm_tt_f8<1, 0>(g, s);
  else if (fmt_a == 0 && fmt_b == 0) launch_gemm_tt_f8<0, 0>(g, s);
  else return -1;
  return (int)hipGetLastError();
}

int gemm_bias_grad(const float* part, int parts, int N, void* out, int odt, hipStream_t s) {
  if (odt == kBF16Code) launch_partial_colsum<bf16>(part, parts, N, N, (bf16*)out, s);
  else if (odt == kF16Code) launch_partial_colsum<f16>(part, parts, N, N, (f16*)out, s);
  else if (odt == kF32Code) launch_partial_colsum<float>(part, parts, N, N, (float*)out, s);
  else return -1;
  return (int)hipGetLastError();
}

int transpose_2d(const void* in, void* out, int R, int C, int dt, hipStream_t s) {
  if (R == 0 || C == 0) return 0;
  dim3 grid((C + 63) / 64, (R + 255) / 256);
  if (dt == kBF16Code)
    hipLaunchKernelGGL((transpose_kernel<bf16>), grid, dim3(256), 0, s, (const bf16*)in, (bf16*)out, R, C);
  else if (dt == kF16Code)
    hipLaunchKernelGGL((transpose_kernel<f16>), grid, dim3(256), 0, s, (const f16*)in, (f16*)out, R, C);
  else
    return -1;
  return (int)hipGetLastError();
}

}  // namespace apex
