// MX quantiser (apex.fp8.mx_quantize): x [R, C] in bf16 / fp16 / fp32 -> OCP Microscaling operands
// for csrc/gemm_mx.hip and csrc/gemm_mx4.hip, 1 x 32 blocks with one E8M0 scale byte each, computed from the block's own
// amax (no history, no per-tensor state). One launch reads x once and writes either or both of
//   rowwise  codes [R, C],  scales [R, C / 32]: blocks of 32 consecutive elements of a row (C % 32 == 0)
//   colwise  codes [C, R],  scales [C, R / 32]: the transposed codes, blocks of 32 consecutive elements
//            of a column of x (R % 32 == 0) — the K-contiguous operand of the input-gradient and
//            weight-gradient GEMMs.
// Contract, to the bit (tests/mx_reference.py computes it in float64), formats e4m3 (OCP fn) / e5m2:
//   amax  = the block's max |x| as fp32; E = its biased exponent field (0 for zero and fp32 subnormals)
//   s     = max(E - emax, 0), emax = 8 (e4m3) / 15 (e5m2): the scale byte, encoding 2^(s - 127)
//   codes = encode(sat(x * 2^(127 - s))), round to nearest even, saturating to +-448 / +-57344: with this
//           rule |x * 2^(127 - s)| < 2^(emax + 1), and [448, 512) / (57344, 65536) saturate (the OCP MX
//           conversion). The multiplication by a power of two is exact; the conversion is fp8_pack.h's
//           v_med3_f32 + v_cvt_pk_{fp8,bf8}_f32.
// Non-finite input: a block holding an inf or a NaN gets the scale byte 0xFF (E8M0 NaN) and its elements
// are converted unscaled (multiplier 1) with the per-tensor quantisers' documented behaviour (fp8.hip):
// +-inf saturates to +-max, a NaN becomes -max (0xfe / 0xfb), finite elements saturate as usual. The
// max is taken over the bit patterns of |x| as integers, which order like the values and put every NaN
// above inf, so E = 255 exactly when the block holds a non-finite element.
// What the scaled MFMA does with a 0xFF scale, measured once on an MI355X (gemm_mx.hip's header,
// tests/test_mx_gpu.py::test_nan_scale): it honours the E8M0 NaN — every output element whose operand
// row has such a block is NaN, whatever the block's codes, and no other element is touched. So a
// non-finite input reaches the GEMM's output as NaN on its row, although its code is a finite one.
//
// Work split: 64 x 64 tiles, 256 threads. A thread loads 16 consecutive elements of a row (two or four
// 16-byte loads), and with its neighbour (lane ^ 1) owns one 32-block: one shuffle for the amax, one
// 16-byte store of 16 codes, one scale byte per pair. For the colwise output the tile's fp32 values go
// through LDS ([64][65]: the column reads of a wave hit 64 different banks), a thread gathers 16
// consecutive rows of one column, and the same pair logic produces 16-byte stores along R.
//
// Format 2, e2m1 (MXFP4; grid +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, emax = 2, max 6): the same contract with
// s = max(E - 2, 0), so |x * 2^(127 - s)| < 8 and (6, 8) saturates to +-6; ties go to the even code; a zero
// keeps its sign. Codes are packed two to a byte, element 2 i in the low nibble: rowwise [R, C / 2], colwise
// [C, R / 2] (packed along R after the LDS transpose). Non-finite blocks: s = 0xFF, multiplier 1, +-inf ->
// +-6, NaN -> 0xF (-6, the "NaN becomes -max" rule), finite values saturate.
// Conversion: v_cvt_scalef32_pk_fp4_f32 with scale 1 (the kernel's own exact power-of-two multiply comes
// first), measured on an MI355X over every tie (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5, both signs), their fp32
// neighbours, the saturating interval, huge values and +-inf: round to nearest even, saturating, the first
// source in the low nibble — the contract bit for bit. A NaN is the exception (the instruction returns the
// maximum with the NaN's own sign bit), so in a non-finite block (E = 255, a wave-rare branch) every NaN
// is replaced by -inf before the conversion.
// Work split for e2m1: the pair scheme is kept — a thread still loads 16 consecutive elements and shares
// the amax with lane ^ 1 — and a thread stores its 8 bytes (a pair 16 contiguous bytes, a row's four threads
// one 32-byte run). Giving a thread a whole 32-block would make the store 16 bytes and drop the shuffle, but
// halve the threads over the same tile and double the fp32 values each holds across the LDS transpose; x is
// read at the same width either way, and the reads are 4 to 8 times the bytes of the stores.
#include "common.h"
#include "fp8_pack.h"
#include "kernels.h"

namespace apex {
namespace {

// 16 values of a block half -> its codes and the block's scale byte; `mb` = max over this half of the
// bit patterns of |v| (combined here with the other half's, held by lane ^ 1)
// (FMT 2, e2m1: the 8 packed bytes are w.x, w.y)
template <int FMT>
__device__ __forceinline__ uint4 mx_encode16(const float (&v)[16], uint32_t mb, int& sbyte) {
  constexpr int EMAX = FMT == 0 ? 8 : FMT == 1 ? 15 : 2;
  const uint32_t ob = (uint32_t)__shfl_xor((int)mb, 1, 64);
  mb = mb > ob ? mb : ob;
  const int E = (int)(mb >> 23);
  sbyte = E == 255 ? 255 : (E > EMAX ? E - EMAX : 0);
  const float mult = E == 255 ? 1.f : __uint_as_float((uint32_t)(254 - sbyte) << 23);
  uint4 w;
  if constexpr (FMT == 2) {
    float p[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) p[k] = v[k] * mult;
    if (E == 255) {
#pragma unroll
      for (int k = 0; k < 16; ++k) p[k] = p[k] != p[k] ? -__builtin_inff() : p[k];
    }
    uint32_t lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(lo, p[0], p[1], 1.f, 0);
    lo = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(lo, p[2], p[3], 1.f, 1);
    lo = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(lo, p[4], p[5], 1.f, 2);
    lo = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(lo, p[6], p[7], 1.f, 3);
    hi = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(hi, p[8], p[9], 1.f, 0);
    hi = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(hi, p[10], p[11], 1.f, 1);
    hi = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(hi, p[12], p[13], 1.f, 2);
    hi = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(hi, p[14], p[15], 1.f, 3);
    w.x = lo, w.y = hi, w.z = 0, w.w = 0;
    return w;
  }
  w.x = f8_pack4<FMT>(v[0] * mult, v[1] * mult, v[2] * mult, v[3] * mult);
  w.y = f8_pack4<FMT>(v[4] * mult, v[5] * mult, v[6] * mult, v[7] * mult);
  w.z = f8_pack4<FMT>(v[8] * mult, v[9] * mult, v[10] * mult, v[11] * mult);
  w.w = f8_pack4<FMT>(v[12] * mult, v[13] * mult, v[14] * mult, v[15] * mult);
  return w;
}

__device__ __forceinline__ uint32_t mx_absmax16(const float (&v)[16]) {
  uint32_t mb = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t b = __float_as_uint(v[k]) & 0x7fffffffu;
    mb = mb > b ? mb : b;
  }
  return mb;
}

template <typename T, int FMT, bool ROW, bool COL>
__global__ void __launch_bounds__(256) mx_quantize_kernel(const T* __restrict__ x, uint8_t* __restrict__ yr,
                                                          uint8_t* __restrict__ sr, uint8_t* __restrict__ yc,
                                                          uint8_t* __restrict__ sc, int R, int C, int tiles_c) {
  __shared__ float tile[COL ? 64 : 1][65];
  const int tid = threadIdx.x;
  const int r0 = (int)(blockIdx.x / tiles_c) * 64, c0 = (int)(blockIdx.x % tiles_c) * 64;
  {
    const int rr = tid >> 2, cg = (tid & 3) * 16;
    const int r = r0 + rr, c = c0 + cg;
    float v[16];
    if (r < R && c + 16 <= C && (C & 15) == 0) {
      const T* p = x + (int64_t)r * C + c;
      constexpr int V = 16 / (int)sizeof(T);  // elements per 16-byte load
#pragma unroll
      for (int q = 0; q < 16 / V; ++q) {
        float t[V];
        load_f<T, V>(p + q * V, t);
#pragma unroll
        for (int k = 0; k < V; ++k) v[q * V + k] = t[k];
      }
    } else {  // a colwise-only launch with C % 16 != 0, or outside the tensor
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = (r < R && c + k < C) ? to_f(x[(int64_t)r * C + c + k]) : 0.f;
    }
    if constexpr (ROW) {  // (C % 32 == 0: the pair's block is inside the row or outside it)
      int sb;
      const uint4 w = mx_encode16<FMT>(v, mx_absmax16(v), sb);
      if (r < R && c < C) {
        if constexpr (FMT == 2) *reinterpret_cast<uint2*>(yr + (((int64_t)r * C + c) >> 1)) = make_uint2(w.x, w.y);
        else *reinterpret_cast<uint4*>(yr + (int64_t)r * C + c) = w;
        if (!(tid & 1)) sr[(int64_t)r * (C >> 5) + (c >> 5)] = (uint8_t)sb;
      }
    }
    if constexpr (COL) {
#pragma unroll
      for (int k = 0; k < 16; ++k) tile[rr][cg + k] = v[k];
    }
  }
  if constexpr (COL) {  // (R % 32 == 0: the pair's 32 rows are inside the tensor or outside it)
    __syncthreads();
    const int cc = tid >> 2, rg = (tid & 3) * 16;
    const int c = c0 + cc, r = r0 + rg;
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = tile[rg + k][cc];
    int sb;
    const uint4 w = mx_encode16<FMT>(v, mx_absmax16(v), sb);
    if (c < C && r < R) {
      if constexpr (FMT == 2) *reinterpret_cast<uint2*>(yc + (((int64_t)c * R + r) >> 1)) = make_uint2(w.x, w.y);
      else *reinterpret_cast<uint4*>(yc + (int64_t)c * R + r) = w;
      if (!(tid & 1)) sc[(int64_t)c * (R >> 5) + (r >> 5)] = (uint8_t)sb;
    }
  }
}

template <typename T, int FMT>
int launch_mxq(const void* x, uint8_t* yr, uint8_t* sr, uint8_t* yc, uint8_t* sc, int R, int C, hipStream_t s) {
  const int tiles_c = (C + 63) / 64;
  const dim3 grid((unsigned)(tiles_c * (int64_t)((R + 63) / 64))), blk(256);
  if (yr && yc) hipLaunchKernelGGL((mx_quantize_kernel<T, FMT, true, true>), grid, blk, 0, s, (const T*)x, yr, sr, yc, sc, R, C, tiles_c);
  else if (yr) hipLaunchKernelGGL((mx_quantize_kernel<T, FMT, true, false>), grid, blk, 0, s, (const T*)x, yr, sr, yc, sc, R, C, tiles_c);
  else hipLaunchKernelGGL((mx_quantize_kernel<T, FMT, false, true>), grid, blk, 0, s, (const T*)x, yr, sr, yc, sc, R, C, tiles_c);
  return (int)hipGetLastError();
}

}  // namespace

bool mx_quantize_supported(int64_t R, int64_t C, bool rowwise, bool colwise) {
  if (R < 1 || C < 1 || !(rowwise || colwise)) return false;
  if ((rowwise && (C & 31)) || (colwise && (R & 31))) return false;
  return R < (1ll << 31) - 64 && C < (1ll << 31) - 64 && ((R + 63) / 64) * ((C + 63) / 64) < (1ll << 31);
}

int mx_quantize(const void* x, int R, int C, int dt, int fmt, uint8_t* yr, uint8_t* sr, uint8_t* yc, uint8_t* sc,
                hipStream_t s) {
  if (!mx_quantize_supported(R, C, yr != nullptr, yc != nullptr) || (yr && !sr) || (yc && !sc) || fmt < 0 || fmt > 2) return -2;
  if (fmt == 2) {
    APEX_DISPATCH_T(dt, T, return (launch_mxq<T, 2>(x, yr, sr, yc, sc, R, C, s)));
  } else if (fmt == 0) {
    APEX_DISPATCH_T(dt, T, return (launch_mxq<T, 0>(x, yr, sr, yc, sc, R, C, s)));
  } else {
    APEX_DISPATCH_T(dt, T, return (launch_mxq<T, 1>(x, yr, sr, yc, sc, R, C, s)));
  }
  return -1;
}

}  // namespace apex
