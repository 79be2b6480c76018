// Fused rotary position embedding (apex.transformer.functional.fused_rope and the GPT models'
// packed-QKV rotation): non-interleaved "rotate half" from fp32-computed cos / sin TABLES, no
// device trig.
//
// Logical tensor [S, B, H, D] with element strides for seq / batch / head on input and output
// (D contiguous), so Apex's sbhd, the project's [B, S, H, D] and slices of packed QKV all run
// without a copy. Table cos, sin : [rows, d2], fp32 or the tensor's dtype, d2 <= D, d2 even.
// With half = d2 / 2 and i < half (the two table halves are NOT assumed equal):
//   forward   y[i]       = x[i] c[i]           - x[i+half] s[i]
//             y[i+half]  = x[i+half] c[i+half] + x[i] s[i+half]
//   backward  dx[i]      = dy[i] c[i]           + dy[i+half] s[i+half]
//             dx[i+half] = dy[i+half] c[i+half] - dy[i] s[i]
// and elements >= d2, heads >= rot_heads (the V third of packed QKV) and thd tokens at or past
// cu_seqlens[-1] are copied bit for bit. Both directions are one expression,
//   out_lo = a c_lo + b sa,   out_hi = b c_hi + a sb
// with (sa, sb) = (-s_lo, s_hi) forward and (s_hi, -s_lo) backward, fixed when the table is loaded.
// All math is fp32, the output is rounded once. No atomics: bitwise repeatable.
//
// thd mode (cu_seqlens != null): tokens [T, H, D] (B = 1), a token's table row is its offset in
// its sequence, found by a binary search over cu_seqlens on the device (uniform per workgroup in
// the vector kernel). The table row is clamped to [0, rows - 1] in every mode, so a too-short
// table or a malformed cu_seqlens cannot read out of bounds.
//
// Vector kernel: one workgroup per token, blockDim = (L, G). Lane x < P = d2 / (2 V) owns the
// V-element chunk at x V and its partner at x V + half (V = 16 bytes of T); lanes >= P own one
// chunk of the unrotated tail. A lane loads its cos / sin once and reuses them over its loop on
// (b, h), so table traffic and conversions are amortised over batch and heads. Everything that
// does not meet the 16-byte conditions takes the scalar kernel with the same semantics.
#include "common.h"
#include "kernels.h"

namespace apex {

namespace {

// table row for token s, and whether the token is rotated at all
__device__ __forceinline__ int64_t rope_row(const RopeArgs& a, int64_t s, bool& live) {
  int64_t row = s;
  live = true;
  if (a.cu_seqlens) {
    const int* cu = a.cu_seqlens;
    live = s < (int64_t)cu[a.nseq];
    // largest j in [0, nseq) with cu[j] <= s (empty sequences are stepped over)
    int lo = 0, hi = a.nseq;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)cu[mid] <= s) lo = mid; else hi = mid;
    }
    row = s - (int64_t)cu[lo];
  }
  row = row < a.rows - 1 ? row : a.rows - 1;
  return row > 0 ? row : 0;
}

template <typename TT, int V>
__device__ __forceinline__ void load_tab(const TT* __restrict__ p, float (&out)[V]) {
  constexpr int N = 16 / (int)sizeof(TT);  // elements per 16-byte load
  static_assert(V % N == 0, "table chunk is whole 16-byte loads");
#pragma unroll
  for (int j = 0; j < V / N; ++j) {
    float t[N];
    load_f<TT, N>(p + j * N, t);
#pragma unroll
    for (int k = 0; k < N; ++k) out[j * N + k] = t[k];
  }
}

template <typename T, typename TT>
__global__ void __launch_bounds__(256) rope_vec_kernel(const RopeArgs a) {
  constexpr int V = 16 / (int)sizeof(T);
  using P16 = Pack<T, V>;
  const int half = a.d2 >> 1;
  const int P = half / V;
  const int c = threadIdx.x;
  const int64_t s = blockIdx.x;
  bool live;
  const int64_t row = rope_row(a, s, live);
  const bool pair = c < P;
  const int lo = pair ? c * V : a.d2 + (c - P) * V;

  float cl[V], ch[V], sa[V], sb[V];
  if (pair) {
    const TT* cp = (const TT*)a.cos + row * a.d2 + lo;
    const TT* sp = (const TT*)a.sin + row * a.d2 + lo;
    float sl[V], sh[V];
    load_tab<TT, V>(cp, cl);
    load_tab<TT, V>(cp + half, ch);
    load_tab<TT, V>(sp, sl);
    load_tab<TT, V>(sp + half, sh);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      sa[k] = a.backward ? sh[k] : -sl[k];
      sb[k] = a.backward ? -sl[k] : sh[k];
    }
  }

  const T* __restrict__ xs = (const T*)a.x + s * a.xs_s + lo;
  T* __restrict__ ys = (T*)a.y + s * a.ys_s + lo;
  const int64_t BH = a.B * a.H;
  const int64_t step = (int64_t)gridDim.y * blockDim.y;
  const int64_t db = step / a.H, dh = step - db * a.H;
  int64_t bh = (int64_t)blockIdx.y * blockDim.y + threadIdx.y;
  int64_t b = bh / a.H, h = bh - b * a.H;
  for (; bh < BH; bh += step) {
    const T* xp = xs + b * a.xs_b + h * a.xs_h;
    T* yp = ys + b * a.ys_b + h * a.ys_h;
    if (pair) {
      const P16 u = *reinterpret_cast<const P16*>(xp);
      const P16 w = *reinterpret_cast<const P16*>(xp + half);
      P16 ou = u, ow = w;
      if (live && h < a.rot_heads) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float uf = to_f(u.v[k]), wf = to_f(w.v[k]);
          ou.v[k] = from_f<T>(uf * cl[k] + wf * sa[k]);
          ow.v[k] = from_f<T>(wf * ch[k] + uf * sb[k]);
        }
      }
      *reinterpret_cast<P16*>(yp) = ou;
      *reinterpret_cast<P16*>(yp + half) = ow;
    } else {
      *reinterpret_cast<P16*>(yp) = *reinterpret_cast<const P16*>(xp);
    }
    b += db;
    h += dh;
    if (h >= a.H) {
      h -= a.H;
      ++b;
    }
  }
}

// One thread per pair (i, i + half) or per tail element; any d2, strides and alignment.
template <typename T, typename TT>
__global__ void __launch_bounds__(256) rope_scalar_kernel(const RopeArgs a) {
  const int half = a.d2 >> 1;
  const int64_t U = (int64_t)half + (a.D - a.d2);  // work items per head
  const int64_t total = a.S * a.B * a.H * U;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int u = (int)(idx % U);
    int64_t r = idx / U;
    const int64_t h = r % a.H;
    r /= a.H;
    const int64_t b = r % a.B, s = r / a.B;
    const T* xp = (const T*)a.x + s * a.xs_s + b * a.xs_b + h * a.xs_h;
    T* yp = (T*)a.y + s * a.ys_s + b * a.ys_b + h * a.ys_h;
    if (u >= half) {
      const int j = a.d2 + (u - half);
      yp[j] = xp[j];
      continue;
    }
    bool live;
    const int64_t row = rope_row(a, s, live);
    const T xu = xp[u], xw = xp[u + half];
    if (!(live && h < a.rot_heads)) {
      yp[u] = xu;
      yp[u + half] = xw;
      continue;
    }
    const TT* cp = (const TT*)a.cos + row * a.d2;
    const TT* sp = (const TT*)a.sin + row * a.d2;
    const float cl = to_f(cp[u]), ch = to_f(cp[u + half]), sl = to_f(sp[u]), sh = to_f(sp[u + half]);
    const float sa = a.backward ? sh : -sl, sb = a.backward ? -sl : sh;
    const float uf = to_f(xu), wf = to_f(xw);
    yp[u] = from_f<T>(uf * cl + wf * sa);
    yp[u + half] = from_f<T>(wf * ch + uf * sb);
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T, typename TT>
int rope_launch(const RopeArgs& a, bool vec, hipStream_t st) {
  if (vec) {
    constexpr int V = 16 / (int)sizeof(T);
    const int L = a.d2 / (2 * V) + (a.D - a.d2) / V;  // lanes per head (<= 256: rope_vector_path)
    int G = 256 / L;                                  // (b, h) pairs in flight per workgroup
    const int64_t BH = a.B * a.H;
    if (G > BH) G = (int)BH;
    // split the (b, h) loop over blockIdx.y only while the token count alone leaves the device
    // short of workgroups; sized from the problem, not from a device query
    const int64_t per = (BH + G - 1) / G;
    int64_t gy = (2048 + a.S - 1) / a.S;
    if (gy > per) gy = per;
    hipLaunchKernelGGL((rope_vec_kernel<T, TT>), dim3((unsigned)a.S, (unsigned)gy), dim3(L, G), 0, st, a);
  } else {
    const int64_t total = a.S * a.B * a.H * ((int64_t)(a.d2 / 2) + (a.D - a.d2));
    int64_t blocks = (total + 255) / 256;
    if (blocks > (1 << 16)) blocks = 1 << 16;
    hipLaunchKernelGGL((rope_scalar_kernel<T, TT>), dim3((unsigned)blocks), dim3(256), 0, st, a);
  }
  return (int)hipGetLastError();
}

template <typename T>
int rope_dispatch_tab(const RopeArgs& a, bool vec, hipStream_t st) {
  if (a.tdt == kF32Code) return rope_launch<T, float>(a, vec, st);
  if (a.tdt == a.dt) return rope_launch<T, T>(a, vec, st);
  return -1;
}

}  // namespace

int rope_vector_path(const RopeArgs& a) {
  const int V = a.dt == kF32Code ? 4 : 8;
  if (a.d2 % (2 * V) || a.D % V) return 0;
  if (a.d2 / (2 * V) + (a.D - a.d2) / V > 256) return 0;
  if (a.S > 0x7fffffffLL) return 0;
  // a stride over a dimension of size 1 is never applied
  const int64_t st[6] = {a.S > 1 ? a.xs_s : 0, a.B > 1 ? a.xs_b : 0, a.H > 1 ? a.xs_h : 0,
                         a.S > 1 ? a.ys_s : 0, a.B > 1 ? a.ys_b : 0, a.H > 1 ? a.ys_h : 0};
  for (int i = 0; i < 6; ++i)
    if (st[i] % V) return 0;
  // table rows are d2 elements: fp32 rows are 16-byte multiples whenever d2 % 4 == 0, rows in a
  // 16-bit dtype need d2 % 8 == 0; both follow from d2 % (2 V) == 0
  return al16(a.x) && al16(a.y) && al16(a.cos) && al16(a.sin);
}

int rope_apply(const RopeArgs& a, hipStream_t st) {
  if (a.S < 0 || a.B < 0 || a.H < 0 || a.D <= 0 || a.d2 < 0 || a.d2 > a.D || (a.d2 & 1) || a.rows < 1) return -2;
  if (a.cu_seqlens && (a.nseq < 1 || a.B != 1)) return -2;
  if (a.S == 0 || a.B == 0 || a.H == 0) return 0;
  const bool vec = rope_vector_path(a) != 0;
  switch (a.dt) {
    case kF32Code: return rope_dispatch_tab<float>(a, vec, st);
    case kF16Code: return rope_dispatch_tab<f16>(a, vec, st);
    case kBF16Code: return rope_dispatch_tab<bf16>(a, vec, st);
  }
  return -1;
}

}  // namespace apex
