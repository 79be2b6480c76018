// Grouped-query attention backward: the sum of the per-query-head dK / dV over each group.
//
// The backward kernels keep one workgroup per (batch, query head) and write dK / dV per query head
// into contiguous [B, Sk, H, D] scratch; this kernel folds the g = H / Hk heads of a group into the
// caller's [B, Sk, Hk, D] gradient (any batch / seq / head strides, so it can be a slice of a packed
// QKV gradient). Memory-bound streaming: one 16-byte piece of one output row per thread, the g source
// pieces D elements apart, fp32 accumulation in ascending head order, one rounding, one 16-byte store.
#include "common.h"
#include "kernels.h"

namespace apex {
namespace {

struct GroupReduceArgs {
  const void* src[2];  // dk_x, dv_x: contiguous [rows * g, D], rows = B * Sk * Hk
  void* dst[2];        // dk, dv
  int64_t bs[2], ss[2], hs[2];
  int64_t pieces;      // rows * (D / N) per tensor
  int Sk, Hk, g, D;
};

template <typename T>
__global__ void __launch_bounds__(256) attn_kv_group_reduce_kernel(GroupReduceArgs a) {
  constexpr int N = 16 / (int)sizeof(T);
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.pieces) return;
  const int t = blockIdx.y;  // 0: dk, 1: dv
  const int ppr = a.D / N;   // pieces per row
  const int64_t row = idx / ppr;
  const int col = (int)(idx - row * ppr) * N;
  const int hk = (int)(row % a.Hk);
  const int64_t bs_ = row / a.Hk;  // b * Sk + s
  const int64_t b = bs_ / a.Sk, s = bs_ - b * a.Sk;

  const T* src = (const T*)a.src[t] + row * a.g * a.D + col;
  float acc[N];
#pragma unroll
  for (int e = 0; e < N; ++e) acc[e] = 0.f;
#pragma unroll 4
  for (int i = 0; i < a.g; ++i) {
    float x[N];
    load_f<T, N>(src + (int64_t)i * a.D, x);
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] += x[e];
  }
  store_f<T, N>((T*)a.dst[t] + b * a.bs[t] + s * a.ss[t] + hk * a.hs[t] + col, acc);
}

}  // namespace

int attn_kv_group_reduce(const void* dk_x, const void* dv_x, void* dk, void* dv, int64_t B, int64_t Sk,
                         int Hk, int g, int D, int64_t dk_bs, int64_t dk_ss, int64_t dk_hs, int64_t dv_bs,
                         int64_t dv_ss, int64_t dv_hs, int dt, hipStream_t s) {
  const int n = dt == kF32 ? 4 : 8;
  if (g < 1 || D <= 0 || D % n != 0 || Hk < 1) return -1;
  GroupReduceArgs a;
  a.src[0] = dk_x, a.src[1] = dv_x;
  a.dst[0] = dk, a.dst[1] = dv;
  a.bs[0] = dk_bs, a.ss[0] = dk_ss, a.hs[0] = dk_hs;
  a.bs[1] = dv_bs, a.ss[1] = dv_ss, a.hs[1] = dv_hs;
  a.pieces = B * Sk * Hk * (D / n);
  a.Sk = (int)Sk, a.Hk = Hk, a.g = g, a.D = D;
  if (a.pieces == 0) return 0;
  const int64_t blocks = (a.pieces + 255) / 256;
  if (blocks > 0x7fffffffLL) return -2;
  const dim3 grid((unsigned)blocks, 2);
  APEX_DISPATCH_T(dt, T, hipLaunchKernelGGL((attn_kv_group_reduce_kernel<T>), grid, dim3(256), 0, s, a));
  return (int)hipGetLastError();
}

}  // namespace apex
