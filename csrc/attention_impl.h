// Flash attention launchers, one instantiation per head dim (attention_d<D>.hip): which forward
// variant and which backward kernels a launch takes. Overview and file map: attention_common.h.
#pragma once
#include "attention_bwd.h"
#include "attention_fwd.h"

namespace apex {

// 16-bit element types only (APEX_DISPATCH_T would instantiate every kernel for fp32 as well;
// fp32 inputs have their own unit, attention_f32.hip)
#define ATTN_DISPATCH(DT, T, ...)                         \
  switch (DT) {                                             \
    case kF16: { using T = f16; __VA_ARGS__; } break;       \
    case kBF16: { using T = bf16; __VA_ARGS__; } break;     \
    default: return -1;                                     \
  }

// The forward's K/V loop (attn_fwd_kernel's SHORT / DB parameters), from what was measured
// (profiles/README.md, "Attention unit split"):
//   single-stage short: D = 64, at most two key tiles, no score bias; with dropout too (253 vs 262-264 us);
//   double-buffered: longer key ranges at D >= 128, and at D = 64 without dropout (with it the
//     two-barrier loop is faster, 87 vs 96 us);
//   two-barrier: everything else.
enum class FwdLoop { kShort, kDoubleBuffered, kTwoBarrier };
constexpr FwdLoop attn_fwd_loop(int D, int Sk, bool dropout, bool bias) {
  const bool long_keys = Sk > 2 * kFwdKB;
  if (D == 64 && !long_keys && !bias) return FwdLoop::kShort;
  if (long_keys && (D >= 128 || (D == 64 && !dropout))) return FwdLoop::kDoubleBuffered;
  return FwdLoop::kTwoBarrier;
}
// whether any key length takes loop L: the others are not instantiated
constexpr bool attn_fwd_reaches(FwdLoop L, int D, bool dropout, bool bias) {
  return attn_fwd_loop(D, 2 * kFwdKB, dropout, bias) == L || attn_fwd_loop(D, 2 * kFwdKB + 1, dropout, bias) == L;
}

template <typename T, int D, bool CAUSAL, bool DROPOUT, bool BIAS, FwdLoop L>
void attn_fwd_launch(const AttnArgs& a, hipStream_t s) {
  // grid (B*H, query blocks), dispatched x-fastest: every head's block of one query range goes out
  // together, and with a causal mask the heaviest ranges (the last query blocks, which see the most
  // keys) go first, so the short blocks fill the tail (longest-first list scheduling)
  const dim3 grid(a.B * a.H, (a.Sq + kFwdBQ - 1) / kFwdBQ);
  if constexpr (attn_fwd_reaches(L, D, DROPOUT, BIAS))
    hipLaunchKernelGGL((attn_fwd_kernel<T, D, CAUSAL, DROPOUT, L == FwdLoop::kShort, BIAS, L == FwdLoop::kDoubleBuffered>),
                       grid, dim3(256), 0, s, a);
}

template <int D>
int attn_fwd_impl(const AttnArgs& a, int dt, hipStream_t s) {
  const bool drop = a.drop_thresh > 0, bias = a.bias != nullptr;
  const FwdLoop loop = attn_fwd_loop(D, a.Sk, drop, bias);  // (k_lens <= Sk)
  ATTN_DISPATCH(dt, T, APEX_DISPATCH_B(a.causal, C, APEX_DISPATCH_B(drop, DR, APEX_DISPATCH_B(bias, BI, {
    switch (loop) {
      case FwdLoop::kShort: attn_fwd_launch<T, D, C, DR, BI, FwdLoop::kShort>(a, s); break;
      case FwdLoop::kDoubleBuffered: attn_fwd_launch<T, D, C, DR, BI, FwdLoop::kDoubleBuffered>(a, s); break;
      case FwdLoop::kTwoBarrier: attn_fwd_launch<T, D, C, DR, BI, FwdLoop::kTwoBarrier>(a, s); break;
    }
  }))));
  return (int)hipGetLastError();
}

// One key block (Sk <= 128): the fused kernel (dK, dV and dQ). Longer key ranges: the delta
// pre-pass, the dK/dV kernel and the dQ kernel. (The three kernels at the short length too measured
// 40-50 % slower: profiles/r3_attn_bwd_split_ab.txt.)
template <int D>
int attn_bwd_impl(const AttnArgs& a, const void* dout, float* delta_ws, void* dk, void* dv, int dt,
                  hipStream_t s) {
  const bool drop = a.drop_thresh > 0;
  const bool multi = attn_bwd_needs_dq_acc(a);
  if (multi && !delta_ws) return -4;
  if (a.bias && a.dsum) return -5;  // (not instantiated: the packed-QKV bias-grad fusion runs without a score bias)
  // (B*H, blocks) grids, heaviest blocks first under a causal mask (see attn_fwd_launch)
  const dim3 kgrid(a.B * a.H, (a.Sk + kBwdBK - 1) / kBwdBK);
  const dim3 qgrid(a.B * a.H, (a.Sq + kFwdBQ - 1) / kFwdBQ);
  const dim3 dgrid((a.Sq * (D / 8) + 255) / 256, a.B * a.H);
  ATTN_DISPATCH(dt, T, APEX_DISPATCH_B(a.causal, C, APEX_DISPATCH_B(drop, DR, APEX_DISPATCH_B(a.bias != nullptr, BI,
      APEX_DISPATCH_B(a.dsum != nullptr, DS, {
    if constexpr (!(BI && DS)) {
      if (multi) hipLaunchKernelGGL((attn_bwd_delta_kernel<T, D>), dgrid, dim3(256), 0, s, a, dout, delta_ws);
      APEX_DISPATCH_B(!multi, DQ,
          hipLaunchKernelGGL((attn_bwd_kernel<T, D, C, DR, DS, DQ, BI>), kgrid, dim3(256), 0, s, a, dout,
                             DQ ? nullptr : (const float*)delta_ws, dk, dv));
      if (multi)
        hipLaunchKernelGGL((attn_bwd_dq_kernel<T, D, C, DR, DS, BI>), qgrid, dim3(256), 0, s, a, dout,
                           (const float*)delta_ws);
    }
  })))));
  return (int)hipGetLastError();
}

// entry points, one translation unit per head dim
int attn_fwd_d32(const AttnArgs& a, int dt, hipStream_t s);
int attn_fwd_d64(const AttnArgs& a, int dt, hipStream_t s);
int attn_fwd_d128(const AttnArgs& a, int dt, hipStream_t s);
int attn_fwd_d256(const AttnArgs& a, int dt, hipStream_t s);
int attn_bwd_d32(const AttnArgs& a, const void* dout, float* delta_ws, void* dk, void* dv, int dt, hipStream_t s);
int attn_bwd_d64(const AttnArgs& a, const void* dout, float* delta_ws, void* dk, void* dv, int dt, hipStream_t s);
int attn_bwd_d128(const AttnArgs& a, const void* dout, float* delta_ws, void* dk, void* dv, int dt, hipStream_t s);
int attn_bwd_d256(const AttnArgs& a, const void* dout, float* delta_ws, void* dk, void* dv, int dt, hipStream_t s);
// fp32 inputs (attention_f32.hip: f32 MFMA), head dims 32 / 64 / 128
int attn_fwd_f32(const AttnArgs& a, hipStream_t s);
int attn_bwd_f32(const AttnArgs& a, const void* dout, float* delta_ws, void* dk, void* dv, hipStream_t s);

}  // namespace apex
