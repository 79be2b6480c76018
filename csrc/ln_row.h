// Row geometry shared by the LayerNorm kernels of layer_norm.hip (ln_*) and fused_ops.hip
// (bdaln_*, embed_ln_*).
//
// One wave64 owns a row (cols % 8 == 0): lane l holds the 16-byte vectors vi = j * 64 + l,
// j < VPT, of which the ones with vi < nvec = cols / 8 are live. A lane therefore always owns the
// same columns, so a backward wave accumulates the column sums (dgamma, dbeta, ...) of all its
// rows in registers, the 4 waves of a block combine them through LDS and the block writes one
// fp32 partial row of the workspace.
//
// The device loops of that scheme stay written out in each kernel; only the formulas that take and
// return plain values are functions here (ln_rstd, ln_dx). Moved behind a function that takes the
// per-lane arrays or an accumulator by reference (a __forceinline__ template, with or without a
// lambda for the kernel's own part), the same statements compile to different code in every kernel
// that calls it: the arrays are promoted to registers in another pass and another order, and
// vectorisation, fma contraction and register assignment follow. profiles/README.md has the table.
#pragma once
#include "common.h"

namespace apex {

constexpr int kLnBlock = 256;  // 4 waves: one row each in forward, interleaved rows in backward

// ------------------------------------ host: geometry --------------------------------------
// 768 blocks = 3 per CU (the 48 KB combine buffer of bdaln at cols 1024 allows 3): 12 waves per
// CU, each with two rows of loads in flight; rows per wave adapts to reach it
constexpr int kLnMaxParts = 768;

// 16-byte vectors per lane for the register-resident kernels: 1 / 2 / 4 (/ 8 where max_vpt allows
// it: only the plain LN forward keeps 8 vectors in registers); 0 = not supported
static inline int ln_vpt(int cols, int max_vpt) {
  if (cols % 8 != 0) return 0;
  const int nvec = cols / 8;
  for (int v = 1; v <= max_vpt; v *= 2)
    if (nvec <= 64 * v) return v;
  return 0;
}

// wide rows, 2056 .. 4096 columns: 5 .. 8 vectors per lane; 0 = not a wide row
static inline int ln_wide_vpt(int cols) {
  if (cols % 8 != 0) return 0;
  const int nvec = cols / 8;
  return (nvec > 256 && nvec <= 512) ? (nvec + 63) / 64 : 0;
}

static inline int ln_rows_per_wave(int64_t rows) {
  const int64_t r = (rows + 4 * kLnMaxParts - 1) / (4 * kLnMaxParts);
  return r < 1 ? 1 : (int)r;
}

// VPT as a constant: the register-resident kernels (1 / 2 / 4, the plain LN forward also 8), the
// wide backward kernels (5 .. 8), and the bdaln forward, which takes either
#define LN_VPT_CASE(N, VPT, ...) case N: { constexpr int VPT = N; __VA_ARGS__; } break;
#define LN_VPT_CASES124(VPT, ...) \
  LN_VPT_CASE(1, VPT, __VA_ARGS__) LN_VPT_CASE(2, VPT, __VA_ARGS__) LN_VPT_CASE(4, VPT, __VA_ARGS__)
#define LN_VPT_CASES567(VPT, ...) \
  LN_VPT_CASE(5, VPT, __VA_ARGS__) LN_VPT_CASE(6, VPT, __VA_ARGS__) LN_VPT_CASE(7, VPT, __VA_ARGS__)
#define LN_DISPATCH_VPT(V, VPT, ...) \
  switch (V) { LN_VPT_CASES124(VPT, __VA_ARGS__) default: return -2; }
#define LN_DISPATCH_VPT8(V, VPT, ...) \
  switch (V) { LN_VPT_CASES124(VPT, __VA_ARGS__) LN_VPT_CASE(8, VPT, __VA_ARGS__) default: return -2; }
#define LN_DISPATCH_VPT_WIDE(V, VPT, ...) \
  switch (V) { LN_VPT_CASES567(VPT, __VA_ARGS__) LN_VPT_CASE(8, VPT, __VA_ARGS__) default: return -2; }
#define LN_DISPATCH_VPT_ANY(V, VPT, ...)                                                       \
  switch (V) {                                                                                 \
    LN_VPT_CASES124(VPT, __VA_ARGS__) LN_VPT_CASES567(VPT, __VA_ARGS__) LN_VPT_CASE(8, VPT, __VA_ARGS__) \
    default: return -2;                                                                        \
  }

// rstd of a row from this lane's share ss of the squared deviations (wave-wide sum inside)
__device__ __forceinline__ float ln_rstd(float ss, float inv_n, float eps) {
  return rsqrtf(wave_sum(ss) * inv_n + eps);
}

// dx of one element from the row means s1 = mean(dy * g), s2 = mean(dy * g * x-hat); dyg = dy * g
template <bool RMS = false>
__device__ __forceinline__ float ln_dx(float dyg, float xh, float rs, float s1, float s2) {
  return RMS ? rs * (dyg - xh * s2) : rs * (dyg - s1 - xh * s2);
}

}  // namespace apex
