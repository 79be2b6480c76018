// Mixture-of-experts token movement: the two row kernels behind moe_permute / moe_unpermute
// (apex/ops/grouped.py), forward and backward.
//
//   moe_gather    out[r, :] = scale[r] * src[row_of[r], :]      r < R; row_of[r] < 0 -> zeros
//   moe_combine   out[t, :] = sum_k w[t, k] * src[dest[t, k], :]
//                 dw[t, k]  = <g[t, :], src[dest[t, k], :]>     (optional, fp32)
//
// permute forward = gather, permute backward = combine without weights, unpermute forward = combine with
// the gate weights, unpermute backward = gather with scale (the row's gate weight) plus combine's dw (the
// gate's gradient). One launch of gather writes all R rows of the expert-sorted tensor, the zero rows
// that pad each segment to a multiple of 64 and the unused tail included, so nothing downstream ever
// reads an uninitialised row.
//
// Work split: one row per wave, four waves per workgroup; lane l moves the 16-byte chunks l, l + 64, ...
// of the row, so every load and store instruction of a wave covers 1 KB of one row. The row index and
// everything read through it (row_of, scale, dest, w) are wave-uniform. The kernels are bound by memory
// traffic and use no LDS; dw is a 6-step wave butterfly. Each output has one writer, combine adds its
// top-k rows in fp32 in the fixed order k = 0, 1, ... and rounds once: results are bit-reproducible.
#include "common.h"
#include "kernels.h"

namespace apex {
namespace {

constexpr int kMoeWaves = 4;

template <typename T>
__global__ void __launch_bounds__(kMoeWaves * 64) moe_gather_kernel(const T* __restrict__ src, const int* __restrict__ row_of,
                                                                    const float* __restrict__ scale, T* __restrict__ out,
                                                                    int R, int S, int H) {
  constexpr int V = 8;  // 16-bit elements per 16-byte chunk
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63;
  const int r = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kMoeWaves + (int)(threadIdx.x >> 6));
  if (r >= R) return;
  const int sr = row_of[r];
  T* o = out + (int64_t)r * H;
  if (sr < 0 || sr >= S) {  // pad / tail row (or an index outside src: zeros, never an access)
    for (int c = lane * V; c < H; c += 64 * V) *reinterpret_cast<u32x4*>(o + c) = u32x4{0u, 0u, 0u, 0u};
    return;
  }
  const T* p = src + (int64_t)sr * H;
  if (scale == nullptr) {  // plain copy: bit-exact
    for (int c = lane * V; c < H; c += 64 * V) *reinterpret_cast<u32x4*>(o + c) = *reinterpret_cast<const u32x4*>(p + c);
    return;
  }
  const float sc = scale[r];
  for (int c = lane * V; c < H; c += 64 * V) {
    float v[V];
    load_f<T, V>(p + c, v);
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] *= sc;
    store_f<T, V>(o + c, v);
  }
}

// out == nullptr: only dw is wanted; g == nullptr: only out
template <typename T>
__global__ void __launch_bounds__(kMoeWaves * 64) moe_combine_kernel(const T* __restrict__ src, const int* __restrict__ dest,
                                                                     const float* __restrict__ w, const T* __restrict__ g,
                                                                     T* __restrict__ out, float* __restrict__ dw, int Tn,
                                                                     int topk, int R, int H) {
  constexpr int V = 8;  // 16-bit elements per 16-byte chunk
  const int lane = threadIdx.x & 63;
  const int t = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kMoeWaves + (int)(threadIdx.x >> 6));
  if (t >= Tn) return;
  float dot[kMoeMaxTopk];
#pragma unroll
  for (int k = 0; k < kMoeMaxTopk; ++k) dot[k] = 0.f;
  for (int c = lane * V; c < H; c += 64 * V) {
    float acc[V], gv[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = gv[i] = 0.f;
    if (g != nullptr) load_f<T, V>(g + (int64_t)t * H + c, gv);
#pragma unroll
    for (int k = 0; k < kMoeMaxTopk; ++k) {
      if (k < topk) {
        const int d = dest[t * topk + k];
        if (d >= 0 && d < R) {  // (an index outside src contributes zero, never an access)
          const float wk = w != nullptr ? w[t * topk + k] : 1.f;
          float v[V];
          load_f<T, V>(src + (int64_t)d * H + c, v);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            acc[i] += wk * v[i];
            dot[k] += gv[i] * v[i];
          }
        }
      }
    }
    if (out != nullptr) store_f<T, V>(out + (int64_t)t * H + c, acc);
  }
  if (g != nullptr) {
#pragma unroll
    for (int k = 0; k < kMoeMaxTopk; ++k) {
      if (k < topk) {
        const float s = wave_sum(dot[k]);
        if (lane == 0) dw[t * topk + k] = s;
      }
    }
  }
}

}  // namespace

bool moe_rows_supported(int64_t rows, int64_t H, int dt) {
  return (dt == kF16 || dt == kBF16) && rows > 0 && H > 0 && H % 8 == 0 && rows < (1ll << 31) - kMoeWaves &&
         H < (1ll << 31);
}

// 16-bit rows only (the dtypes the grouped GEMMs between these kernels run in)
#define MOE_DISPATCH_T(DT, T, ...)                      \
  if (DT == kF16) { using T = f16; __VA_ARGS__; }       \
  else { using T = bf16; __VA_ARGS__; }

int moe_gather(const void* src, const int* row_of, const float* scale, void* out, int R, int S, int H, int dt,
               hipStream_t s) {
  if (!moe_rows_supported(R, H, dt) || S <= 0) return -2;
  const dim3 grid((R + kMoeWaves - 1) / kMoeWaves);
  MOE_DISPATCH_T(dt, T, hipLaunchKernelGGL((moe_gather_kernel<T>), grid, dim3(kMoeWaves * 64), 0, s, (const T*)src,
                                            row_of, scale, (T*)out, R, S, H));
  return (int)hipGetLastError();
}

int moe_combine(const void* src, const int* dest, const float* w, const void* g, void* out, float* dw, int Tn, int topk,
                int R, int H, int dt, hipStream_t s) {
  if (!moe_rows_supported(Tn, H, dt) || R <= 0 || topk < 1 || topk > kMoeMaxTopk || (int64_t)Tn * topk >= (1ll << 31))
    return -2;
  if ((g != nullptr) != (dw != nullptr) || (out == nullptr && g == nullptr)) return -3;
  const dim3 grid((Tn + kMoeWaves - 1) / kMoeWaves);
  MOE_DISPATCH_T(dt, T, hipLaunchKernelGGL((moe_combine_kernel<T>), grid, dim3(kMoeWaves * 64), 0, s, (const T*)src, dest,
                                            w, (const T*)g, (T*)out, dw, Tn, topk, R, H));
  return (int)hipGetLastError();
}

}  // namespace apex
