// Weight norm (K-03), LSTM/GRU cell pointwise (K-06) and SyncBatchNorm (NS-04) kernels.
//
// Weight norm  w = g * v / ||v||, norm over every dim except `dim`:
//   dim == 0   -> "row" layout [R, C] (one norm per row): one 256-thread block per row,
//                 two passes over the row (the second from L2);
//   dim == last-> "col" layout [R, C] (one norm per column): each thread owns one column and
//                 walks the rows (coalesced across threads), fp32 accumulation.
// LSTM / GRU cells: everything after the two GEMMs of a step in ONE kernel each way
// (gate bias adds, sigmoid/tanh, cell update), fp32 math, gate grads written once so the
// caller's GEMMs produce dx/dh/dW; bias grads come from colsum of the gate grads.
// SyncBN: per-channel Welford partials (NCHW or NHWC), combine to global mean/invstd after
// the caller's all-reduce/all-gather, fused normalise(+ReLU), backward reductions
// (sum dy, sum dy*(x-mean)) and the elementwise dx.
#include "common.h"
#include "kernels.h"

namespace apex {


// ============================ weight norm ===================================
template <typename T, typename G>
__global__ void __launch_bounds__(256) wn_row_fwd(const T* __restrict__ v, const G* __restrict__ g,
                                                 T* __restrict__ w, float* __restrict__ norms, int64_t C) {
  __shared__ float red[4];
  const int64_t r = blockIdx.x;
  const T* vr = v + r * C;
  float s = 0.f;
  for (int64_t c = threadIdx.x; c < C; c += 256) {
    const float x = to_f(vr[c]);
    s += x * x;
  }
  const float n = sqrtf(block_sum(s, red));
  if (threadIdx.x == 0) norms[r] = n;
  const float sc = to_f(g[r]) / n;
  T* wr = w + r * C;
  for (int64_t c = threadIdx.x; c < C; c += 256) wr[c] = from_f<T>(to_f(vr[c]) * sc);
}

template <typename T, typename G>
__global__ void __launch_bounds__(256) wn_row_bwd(const T* __restrict__ dw, const T* __restrict__ v,
                                                 const G* __restrict__ g, const float* __restrict__ norms,
                                                 T* __restrict__ dv, G* __restrict__ dg, int64_t C) {
  __shared__ float red[4];
  const int64_t r = blockIdx.x;
  const T* vr = v + r * C;
  const T* dwr = dw + r * C;
  float s = 0.f;
  for (int64_t c = threadIdx.x; c < C; c += 256) s += to_f(dwr[c]) * to_f(vr[c]);
  const float dot = block_sum(s, red);
  const float n = norms[r], gv = to_f(g[r]);
  if (threadIdx.x == 0) dg[r] = from_f<G>(dot / n);
  const float a = gv / n, b = gv * dot / (n * n * n);
  T* dvr = dv + r * C;
  for (int64_t c = threadIdx.x; c < C; c += 256) dvr[c] = from_f<T>(a * to_f(dwr[c]) - b * to_f(vr[c]));
}

template <typename T, typename G>
__global__ void __launch_bounds__(256) wn_col_fwd(const T* __restrict__ v, const G* __restrict__ g,
                                                 T* __restrict__ w, float* __restrict__ norms, int64_t R,
                                                 int64_t C) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int64_t r = 0; r < R; ++r) {
    const float x = to_f(v[r * C + c]);
    s += x * x;
  }
  const float n = sqrtf(s);
  norms[c] = n;
  const float sc = to_f(g[c]) / n;
  for (int64_t r = 0; r < R; ++r) w[r * C + c] = from_f<T>(to_f(v[r * C + c]) * sc);
}

template <typename T, typename G>
__global__ void __launch_bounds__(256) wn_col_bwd(const T* __restrict__ dw, const T* __restrict__ v,
                                                 const G* __restrict__ g, const float* __restrict__ norms,
                                                 T* __restrict__ dv, G* __restrict__ dg, int64_t R,
                                                 int64_t C) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int64_t r = 0; r < R; ++r) s += to_f(dw[r * C + c]) * to_f(v[r * C + c]);
  const float n = norms[c], gv = to_f(g[c]);
  dg[c] = from_f<G>(s / n);
  const float a = gv / n, b = gv * s / (n * n * n);
  for (int64_t r = 0; r < R; ++r) dv[r * C + c] = from_f<T>(a * to_f(dw[r * C + c]) - b * to_f(v[r * C + c]));
}

int weight_norm_fwd(const void* v, const void* g, void* w, float* norms, int64_t R, int64_t C, int row_mode,
                    int vdt, int gdt, hipStream_t s) {
  if (R == 0 || C == 0) return 0;
  APEX_DISPATCH_T(vdt, T, APEX_DISPATCH_T(gdt, G, {
    if (row_mode)
      hipLaunchKernelGGL((wn_row_fwd<T, G>), dim3((unsigned)R), dim3(256), 0, s, (const T*)v, (const G*)g,
                         (T*)w, norms, C);
    else
      hipLaunchKernelGGL((wn_col_fwd<T, G>), dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (const T*)v,
                         (const G*)g, (T*)w, norms, R, C);
  }));
  return (int)hipGetLastError();
}

int weight_norm_bwd(const void* dw, const void* v, const void* g, const float* norms, void* dv, void* dg,
                    int64_t R, int64_t C, int row_mode, int vdt, int gdt, hipStream_t s) {
  if (R == 0 || C == 0) return 0;
  APEX_DISPATCH_T(vdt, T, APEX_DISPATCH_T(gdt, G, {
    if (row_mode)
      hipLaunchKernelGGL((wn_row_bwd<T, G>), dim3((unsigned)R), dim3(256), 0, s, (const T*)dw, (const T*)v,
                         (const G*)g, norms, (T*)dv, (G*)dg, C);
    else
      hipLaunchKernelGGL((wn_col_bwd<T, G>), dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s,
                         (const T*)dw, (const T*)v, (const G*)g, norms, (T*)dv, (G*)dg, R, C);
  }));
  return (int)hipGetLastError();
}

// ============================ RNN cells ======================================
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }

// LSTM: gates [B, 4H] in PyTorch order (i, f, g, o). ws saves activated gates + tanh(cy).
template <typename T>
__global__ void __launch_bounds__(256) lstm_fwd_kernel(const T* __restrict__ ig, const T* __restrict__ hg,
                                                      const T* __restrict__ bih, const T* __restrict__ bhh,
                                                      const T* __restrict__ cx, T* __restrict__ hy,
                                                      T* __restrict__ cy, float* __restrict__ ws, int64_t B,
                                                      int64_t H) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * H) return;
  const int64_t b = idx / H, j = idx % H;
  float pre[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t o = b * 4 * H + k * H + j;
    float v = to_f(ig[o]) + (hg ? to_f(hg[o]) : 0.f);
    if (bih) v += to_f(bih[k * H + j]);
    if (bhh) v += to_f(bhh[k * H + j]);
    pre[k] = v;
  }
  const float i = sigm(pre[0]), f = sigm(pre[1]), g = tanhf(pre[2]), o = sigm(pre[3]);
  const float c = f * to_f(cx[idx]) + i * g;
  const float tc = tanhf(c);
  cy[idx] = from_f<T>(c);
  hy[idx] = from_f<T>(o * tc);
  if (ws) {
    float* w = ws + b * 5 * H;
    w[j] = i;
    w[H + j] = f;
    w[2 * H + j] = g;
    w[3 * H + j] = o;
    w[4 * H + j] = tc;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) lstm_bwd_kernel(const T* __restrict__ dhy, const T* __restrict__ dcy,
                                                      const T* __restrict__ cx, const float* __restrict__ ws,
                                                      T* __restrict__ dgates, T* __restrict__ dcx, int64_t B,
                                                      int64_t H) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * H) return;
  const int64_t b = idx / H, j = idx % H;
  const float* w = ws + b * 5 * H;
  const float i = w[j], f = w[H + j], g = w[2 * H + j], o = w[3 * H + j], tc = w[4 * H + j];
  const float dh = dhy ? to_f(dhy[idx]) : 0.f;
  const float dc = (dcy ? to_f(dcy[idx]) : 0.f) + dh * o * (1.f - tc * tc);
  T* dg = dgates + b * 4 * H;
  dg[j] = from_f<T>(dc * g * i * (1.f - i));
  dg[H + j] = from_f<T>(dc * to_f(cx[idx]) * f * (1.f - f));
  dg[2 * H + j] = from_f<T>(dc * i * (1.f - g * g));
  dg[3 * H + j] = from_f<T>(dh * tc * o * (1.f - o));
  dcx[idx] = from_f<T>(dc * f);
}

// GRU: gates [B, 3H] order (r, z, n). ws saves r, z, n, (hg_n + b_hn).
template <typename T>
__global__ void __launch_bounds__(256) gru_fwd_kernel(const T* __restrict__ ig, const T* __restrict__ hg,
                                                     const T* __restrict__ bih, const T* __restrict__ bhh,
                                                     const T* __restrict__ hx, T* __restrict__ hy,
                                                     float* __restrict__ ws, int64_t B, int64_t H) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * H) return;
  const int64_t b = idx / H, j = idx % H;
  auto IG = [&](int k) { return to_f(ig[b * 3 * H + k * H + j]) + (bih ? to_f(bih[k * H + j]) : 0.f); };
  auto HG = [&](int k) { return to_f(hg[b * 3 * H + k * H + j]) + (bhh ? to_f(bhh[k * H + j]) : 0.f); };
  const float r = sigm(IG(0) + HG(0));
  const float z = sigm(IG(1) + HG(1));
  const float hn = HG(2);
  const float n = tanhf(IG(2) + r * hn);
  const float h = to_f(hx[idx]);
  hy[idx] = from_f<T>((1.f - z) * n + z * h);
  if (ws) {
    float* w = ws + b * 4 * H;
    w[j] = r;
    w[H + j] = z;
    w[2 * H + j] = n;
    w[3 * H + j] = hn;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) gru_bwd_kernel(const T* __restrict__ dhy, const T* __restrict__ hx,
                                                     const float* __restrict__ ws, T* __restrict__ dig,
                                                     T* __restrict__ dhg, T* __restrict__ dhx, int64_t B,
                                                     int64_t H) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * H) return;
  const int64_t b = idx / H, j = idx % H;
  const float* w = ws + b * 4 * H;
  const float r = w[j], z = w[H + j], n = w[2 * H + j], hn = w[3 * H + j];
  const float dh = to_f(dhy[idx]), h = to_f(hx[idx]);
  const float dn = dh * (1.f - z) * (1.f - n * n);
  const float dz = dh * (h - n) * z * (1.f - z);
  const float dr = dn * hn * r * (1.f - r);
  T* di = dig + b * 3 * H;
  T* dhh = dhg + b * 3 * H;
  di[j] = from_f<T>(dr);
  di[H + j] = from_f<T>(dz);
  di[2 * H + j] = from_f<T>(dn);
  dhh[j] = from_f<T>(dr);
  dhh[H + j] = from_f<T>(dz);
  dhh[2 * H + j] = from_f<T>(dn * r);
  dhx[idx] = from_f<T>(dh * z);
}

int lstm_cell_fwd(const void* ig, const void* hg, const void* bih, const void* bhh, const void* cx, void* hy,
                  void* cy, float* ws, int64_t B, int64_t H, int dt, hipStream_t s) {
  const int64_t n = B * H;
  if (n == 0) return 0;
  APEX_DISPATCH_T(dt, T,
      hipLaunchKernelGGL((lstm_fwd_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                         (const T*)ig, (const T*)hg, (const T*)bih, (const T*)bhh, (const T*)cx, (T*)hy,
                         (T*)cy, ws, B, H));
  return (int)hipGetLastError();
}

int lstm_cell_bwd(const void* dhy, const void* dcy, const void* cx, const float* ws, void* dgates, void* dcx,
                  int64_t B, int64_t H, int dt, hipStream_t s) {
  const int64_t n = B * H;
  if (n == 0) return 0;
  APEX_DISPATCH_T(dt, T,
      hipLaunchKernelGGL((lstm_bwd_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                         (const T*)dhy, (const T*)dcy, (const T*)cx, ws, (T*)dgates, (T*)dcx, B, H));
  return (int)hipGetLastError();
}

int gru_cell_fwd(const void* ig, const void* hg, const void* bih, const void* bhh, const void* hx, void* hy,
                 float* ws, int64_t B, int64_t H, int dt, hipStream_t s) {
  const int64_t n = B * H;
  if (n == 0) return 0;
  APEX_DISPATCH_T(dt, T,
      hipLaunchKernelGGL((gru_fwd_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                         (const T*)ig, (const T*)hg, (const T*)bih, (const T*)bhh, (const T*)hx, (T*)hy, ws,
                         B, H));
  return (int)hipGetLastError();
}

int gru_cell_bwd(const void* dhy, const void* hx, const float* ws, void* dig, void* dhg, void* dhx, int64_t B,
                 int64_t H, int dt, hipStream_t s) {
  const int64_t n = B * H;
  if (n == 0) return 0;
  APEX_DISPATCH_T(dt, T,
      hipLaunchKernelGGL((gru_bwd_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                         (const T*)dhy, (const T*)hx, ws, (T*)dig, (T*)dhg, (T*)dhx, B, H));
  return (int)hipGetLastError();
}

// ============================ SyncBatchNorm ==================================
// Layout: NCHW -> element (n, c, s) at n*C*S + c*S + s ; NHWC -> (n*S + s)*C + c.
struct Welford {
  float mean, m2, n;
};
__device__ __forceinline__ Welford wf_merge(Welford a, Welford b) {
  const float n = a.n + b.n;
  if (n == 0.f) return a;
  const float d = b.mean - a.mean;
  const float wb = b.n / n;
  Welford r;
  r.mean = a.mean + d * wb;
  r.m2 = a.m2 + b.m2 + d * d * a.n * wb;
  r.n = n;
  return r;
}

// grid (C, splits): partial Welford of channel c over its slice of the N*S elements
template <typename T>
__global__ void __launch_bounds__(256) bn_stats_kernel(const T* __restrict__ x, float* __restrict__ part,
                                                      int64_t N, int64_t C, int64_t S, int nhwc) {
  __shared__ float sm[3][4];
  const int64_t c = blockIdx.x;
  const int64_t total = N * S;
  const int64_t per = (total + gridDim.y - 1) / gridDim.y;
  const int64_t e0 = (int64_t)blockIdx.y * per, e1 = min(e0 + per, total);
  Welford w{0.f, 0.f, 0.f};
  for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
    const int64_t n = e / S, s2 = e % S;
    const float v = to_f(nhwc ? x[e * C + c] : x[(n * C + c) * S + s2]);
    w.n += 1.f;
    const float d = v - w.mean;
    w.mean += d / w.n;
    w.m2 += d * (v - w.mean);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Welford b{__shfl_xor(w.mean, o, 64), __shfl_xor(w.m2, o, 64), __shfl_xor(w.n, o, 64)};
    w = wf_merge(w, b);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    sm[0][wid] = w.mean;
    sm[1][wid] = w.m2;
    sm[2][wid] = w.n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Welford t{sm[0][0], sm[1][0], sm[2][0]};
    for (int k = 1; k < 4; ++k) t = wf_merge(t, Welford{sm[0][k], sm[1][k], sm[2][k]});
    float* p = part + (c * gridDim.y + blockIdx.y) * 3;
    p[0] = t.mean;
    p[1] = t.m2;
    p[2] = t.n;
  }
}

// combine `groups` Welford triples per channel: in[(g*C + c)*3 ...] (g-major, e.g. all-gathered)
// or in[(c*groups + g)*3] (c-major, local splits). Writes mean, biased var, count per channel.
// The combine's tail for one channel: the global mean / biased variance / count, and optionally
// invstd = rsqrt(var + eps) and the momentum update of the fp32 running statistics (unbiased
// variance) — the 8-10 small torch launches per BatchNorm layer that otherwise follow the combine.
struct BnFinish {
  float* invstd;
  float* rmean;
  float* rvar;
  float* triple;    // [C, 3] (mean, m2, count): the per-rank record all-gathered by SyncBatchNorm
  int64_t* ntrack;  // num_batches_tracked += 1 (channel 0)
  float eps, momentum;
};
__device__ __forceinline__ void bn_finish(const Welford& r, int64_t c, float* mean, float* var, float* count,
                                          const BnFinish& f) {
  const float v = r.n > 0.f ? r.m2 / r.n : 0.f;
  if (mean) mean[c] = r.mean;
  if (var) var[c] = v;
  if (count) count[c] = r.n;
  if (f.triple) {
    f.triple[c * 3] = r.mean;
    f.triple[c * 3 + 1] = r.m2;
    f.triple[c * 3 + 2] = r.n;
  }
  if (f.ntrack && c == 0) f.ntrack[0] += 1;
  if (f.invstd) f.invstd[c] = rsqrtf(v + f.eps);
  if (f.rmean) {
    const float m = f.momentum;
    f.rmean[c] = (1.f - m) * f.rmean[c] + m * r.mean;
    f.rvar[c] = (1.f - m) * f.rvar[c] + m * (v * r.n / fmaxf(r.n - 1.f, 1.f));
  }
}

__global__ void bn_combine_kernel(const float* __restrict__ in, int groups, int64_t C, int gmajor,
                                  float* __restrict__ mean, float* __restrict__ var, float* __restrict__ count,
                                  BnFinish fin) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  Welford t{0.f, 0.f, 0.f};
  for (int g = 0; g < groups; ++g) {
    const float* p = in + (gmajor ? ((int64_t)g * C + c) : (c * groups + g)) * 3;
    t = wf_merge(t, Welford{p[0], p[1], p[2]});
  }
  bn_finish(t, c, mean, var, count, fin);
}

template <typename T, typename W>
__global__ void __launch_bounds__(256) bn_elemt_kernel(const T* __restrict__ x, const float* __restrict__ mean,
                                                      const float* __restrict__ invstd, const W* __restrict__ w,
                                                      const W* __restrict__ b, const T* __restrict__ z,
                                                      T* __restrict__ y, int64_t N, int64_t C, int64_t S, int nhwc,
                                                      int relu) {
  const int64_t total = N * C * S;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t c = nhwc ? e % C : (e / S) % C;
    float v = (to_f(x[e]) - mean[c]) * invstd[c];
    if (w) v *= to_f(w[c]);
    if (b) v += to_f(b[c]);
    if (z) v += to_f(z[e]);
    if (relu) v = fmaxf(v, 0.f);
    y[e] = from_f<T>(v);
  }
}

// partial sums per channel: sum(dy), sum(dy * (x - mean)) ; grid (C, splits)
template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                           const T* __restrict__ ym, const float* __restrict__ mean,
                                                           float* __restrict__ part, int64_t N, int64_t C,
                                                           int64_t S, int nhwc) {
  __shared__ float red[4];
  const int64_t c = blockIdx.x;
  const int64_t total = N * S;
  const int64_t per = (total + gridDim.y - 1) / gridDim.y;
  const int64_t e0 = (int64_t)blockIdx.y * per, e1 = min(e0 + per, total);
  const float mu = mean[c];
  float s1 = 0.f, s2 = 0.f;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
    const int64_t n = e / S, s3 = e % S;
    const int64_t off = nhwc ? e * C + c : (n * C + c) * S + s3;
    const float d = ym && !(to_f(ym[off]) > 0.f) ? 0.f : to_f(dy[off]);
    s1 += d;
    s2 += d * (to_f(x[off]) - mu);
  }
  s1 = block_sum(s1, red);
  s2 = block_sum(s2, red);
  if (threadIdx.x == 0) {
    part[(c * gridDim.y + blockIdx.y) * 2] = s1;
    part[(c * gridDim.y + blockIdx.y) * 2 + 1] = s2;
  }
}

__global__ void bn_bwd_finalize_kernel(const float* __restrict__ part, int splits, int64_t C,
                                       float* __restrict__ sum_dy, float* __restrict__ sum_dy_xmu) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float a = 0.f, b = 0.f;
  for (int k = 0; k < splits; ++k) {
    a += part[(c * splits + k) * 2];
    b += part[(c * splits + k) * 2 + 1];
  }
  sum_dy[c] = a;
  sum_dy_xmu[c] = b;
}

// dx = (dy - mean_dy - (x-mean)*invstd^2*mean_dy_xmu) * invstd * w ; count[c] = global element count
// of channel c, read on the device (the combine kernel's output: no host round trip per layer)
template <typename T, typename W>
__global__ void __launch_bounds__(256) bn_bwd_elemt_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ invstd,
                                                          const W* __restrict__ w, const float* __restrict__ sum_dy,
                                                          const float* __restrict__ sum_dy_xmu,
                                                          const float* __restrict__ count,
                                                          const T* __restrict__ ym, T* __restrict__ dz,
                                                          T* __restrict__ dx, int64_t N, int64_t C, int64_t S,
                                                          int nhwc) {
  const int64_t total = N * C * S;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t c = nhwc ? e % C : (e / S) % C;
    const float is = invstd[c];
    const float inv_count = 1.f / fmaxf(count[c], 1.f);
    const float mdy = sum_dy[c] * inv_count, mdx = sum_dy_xmu[c] * inv_count;
    const float xm = to_f(x[e]) - mean[c];
    const float g = ym && !(to_f(ym[e]) > 0.f) ? 0.f : to_f(dy[e]);
    if (dz) dz[e] = from_f<T>(g);
    float v = (g - mdy - xm * is * is * mdx) * is;
    if (w) v *= to_f(w[c]);
    dx[e] = from_f<T>(v);
  }
}

// ---------------------------------------------------------------------------
// Vectorised SyncBN kernels (16-byte accesses: VEC = 8 for 16-bit data, 4 for fp32). The scalar
// kernels above (one 2-byte element per thread, 64-bit div/mod per element) ran at 1.1-2.7 TB/s
// by rocprofv3 FETCH/WRITE_SIZE (profiles/r2_pmc_bw_kernels.json) and NHWC's per-channel strided
// gather was worse; they remain for shapes these do not take (plane or channel count not a
// multiple of VEC, misaligned views).
//
//  NCHW: a vector = VEC consecutive elements of one channel plane (needs S % VEC == 0).
//  NHWC: a vector = VEC consecutive channels of one row (needs C % VEC == 0); a block covers
//        cvb channel vectors x rpb row lanes and combines its row lanes through LDS.
// Partials keep the layouts of the scalar kernels: Welford triples part[(c*splits + y)*3] for
// bn_combine, (sum_dy, sum_dy_xmu) pairs part[(c*splits + y)*2] for bn_bwd_finalize.
// ---------------------------------------------------------------------------
template <typename T>
struct BnVec {
  static constexpr int V = 16 / (int)sizeof(T);
  typedef Pack<T, V> P;
};

// Welford merge of a VEC-element chunk given its sum / sum of squared deviations
__device__ __forceinline__ void wf_add_chunk(Welford& w, float csum, float cm2, float cn) {
  w = wf_merge(w, Welford{csum / cn, cm2, cn});
}

template <typename T>
__global__ void __launch_bounds__(256) bn_stats_nchw_vec(const T* __restrict__ x, float* __restrict__ part,
                                                        int N, int C, int S) {
  constexpr int V = BnVec<T>::V;
  typedef typename BnVec<T>::P P;
  __shared__ float sm[3][4];
  const int c = blockIdx.x;
  const int SV = S / V;
  const int total = N * SV;
  const int per = (total + gridDim.y - 1) / gridDim.y;
  const int e0 = blockIdx.y * per, e1 = min(e0 + per, total);
  Welford w{0.f, 0.f, 0.f};
  for (int e = e0 + threadIdx.x; e < e1; e += 256) {
    const int n = e / SV, sv = e - n * SV;
    const P pk = *reinterpret_cast<const P*>(x + ((int64_t)n * C + c) * S + (int64_t)sv * V);
    float v[V], cs = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      v[k] = to_f(pk.v[k]);
      cs += v[k];
    }
    const float cm = cs * (1.f / V);
    float m2 = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k) m2 += (v[k] - cm) * (v[k] - cm);
    wf_add_chunk(w, cs, m2, (float)V);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Welford b{__shfl_xor(w.mean, o, 64), __shfl_xor(w.m2, o, 64), __shfl_xor(w.n, o, 64)};
    w = wf_merge(w, b);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    sm[0][wid] = w.mean;
    sm[1][wid] = w.m2;
    sm[2][wid] = w.n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Welford t{sm[0][0], sm[1][0], sm[2][0]};
    for (int k = 1; k < 4; ++k) t = wf_merge(t, Welford{sm[0][k], sm[1][k], sm[2][k]});
    float* p = part + ((int64_t)c * gridDim.y + blockIdx.y) * 3;
    p[0] = t.mean;
    p[1] = t.m2;
    p[2] = t.n;
  }
}

// NHWC: rows R = N*S of C channels. Thread (cv, rl): channel vector cv, rows rl, rl + rpb*splits, ...
template <typename T>
__global__ void __launch_bounds__(256) bn_stats_nhwc_vec(const T* __restrict__ x, float* __restrict__ part,
                                                        int64_t R, int C, int cvb, int rpb) {
  constexpr int V = BnVec<T>::V;
  typedef typename BnVec<T>::P P;
  __shared__ float sm[256 * V * 2 + 256];
  const int CV = C / V;
  const int tc = threadIdx.x % cvb, tr = threadIdx.x / cvb;
  const int cv = blockIdx.x * cvb + tc;
  const bool act = tr < rpb && cv < CV;
  float mean[V], m2[V], n = 0.f;
#pragma unroll
  for (int k = 0; k < V; ++k) mean[k] = m2[k] = 0.f;
  if (act) {
    const int64_t step = (int64_t)rpb * gridDim.y;
    int64_t r = (int64_t)blockIdx.y * rpb + tr;
    // two rows per iteration: two independent 16-byte loads in flight per thread (four measured
    // slower on the ResNet-50 shapes: 38.7 vs 34.7 us average)
    constexpr int U = 2;
    for (; r + (U - 1) * step < R; r += U * step) {
      P a[U];
#pragma unroll
      for (int u = 0; u < U; ++u) a[u] = *reinterpret_cast<const P*>(x + (r + u * step) * C + (int64_t)cv * V);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        n += 1.f;
        const float inv = 1.f / n;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float v = to_f(a[u].v[k]), d = v - mean[k];
          mean[k] += d * inv;
          m2[k] += d * (v - mean[k]);
        }
      }
    }
    for (; r < R; r += step) {
      const P a = *reinterpret_cast<const P*>(x + r * C + (int64_t)cv * V);
      n += 1.f;
      const float inv = 1.f / n;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float v = to_f(a.v[k]), d = v - mean[k];
        mean[k] += d * inv;
        m2[k] += d * (v - mean[k]);
      }
    }
  }
  // combine the rpb row lanes of every channel vector
  float* smean = sm;
  float* sm2 = sm + 256 * V;
  float* sn = sm + 512 * V;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    smean[threadIdx.x * V + k] = mean[k];
    sm2[threadIdx.x * V + k] = m2[k];
  }
  sn[threadIdx.x] = n;
  __syncthreads();
  if (tr == 0 && cv < CV) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      Welford t{smean[tc * V + k], sm2[tc * V + k], sn[tc]};
      for (int q = 1; q < rpb; ++q) {
        const int id = q * cvb + tc;
        t = wf_merge(t, Welford{smean[id * V + k], sm2[id * V + k], sn[id]});
      }
      float* p = part + ((int64_t)(cv * V + k) * gridDim.y + blockIdx.y) * 3;
      p[0] = t.mean;
      p[1] = t.m2;
      p[2] = t.n;
    }
  }
}

// per-channel affine coefficients of the elementwise passes (one thread per channel):
//   forward   y  = x * k0 + k1                     k0 = w * invstd, k1 = b - mean * k0
//   backward  dx = dy * k0 + x * k1 + k2           k0 = w * invstd, k1 = -k0 * invstd^2 * mdx,
//                                                  k2 = k0 * (mean * invstd^2 * mdx - mdy)
// so the vector kernels load 2-3 floats per channel instead of recomputing from 4-7 inputs.
template <typename W>
__global__ void bn_coef_fwd_kernel(const float* __restrict__ mean, const float* __restrict__ invstd,
                                   const W* __restrict__ w, const W* __restrict__ b, float* __restrict__ k, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float k0 = (w ? to_f(w[c]) : 1.f) * invstd[c];
  k[c] = k0;
  k[C + c] = (b ? to_f(b[c]) : 0.f) - mean[c] * k0;
}

template <typename W>
__global__ void bn_coef_bwd_kernel(const float* __restrict__ mean, const float* __restrict__ invstd,
                                   const W* __restrict__ w, const float* __restrict__ sum_dy,
                                   const float* __restrict__ sum_dy_xmu, const float* __restrict__ count,
                                   float* __restrict__ k, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float is = invstd[c], ic = 1.f / fmaxf(count[c], 1.f);
  const float mdy = sum_dy[c] * ic, mdx = sum_dy_xmu[c] * ic;
  const float k0 = (w ? to_f(w[c]) : 1.f) * is;
  const float q = is * is * mdx;
  k[c] = k0;
  k[C + c] = -k0 * q;
  k[2 * C + c] = k0 * (mean[c] * q - mdy);
}

template <int V>
__device__ __forceinline__ void load_coef(const float* __restrict__ k, int c0, float (&o)[V]) {
  if constexpr (V == 8) {
    const float4 a = *reinterpret_cast<const float4*>(k + c0);
    const float4 b = *reinterpret_cast<const float4*>(k + c0 + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  } else {
    const float4 a = *reinterpret_cast<const float4*>(k + c0);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
  }
}

// nvec < 2^31 (checked by the launcher): 32-bit index math
template <typename T>
__global__ void __launch_bounds__(256) bn_elemt_vec(const T* __restrict__ x, const float* __restrict__ k,
                                                   const T* __restrict__ z, T* __restrict__ y, int nvec, int C, int S,
                                                   int nhwc, int relu) {
  constexpr int V = BnVec<T>::V;
  typedef typename BnVec<T>::P P;
  const int SV = S / V, CV = C / V;
  // NHWC with a grid stride that is a multiple of the channel-vector count: every iteration of a
  // thread touches the same channels, so its coefficients are loaded once (per-element loads put
  // 64 B of coefficient fetches through the vector memory pipe for every 16 B of data)
  const bool hoist = nhwc && ((int64_t)gridDim.x * 256) % CV == 0;
  float k0[V], k1[V];
  if (hoist) {
    const int c0 = ((blockIdx.x * 256 + threadIdx.x) % CV) * V;
    load_coef<V>(k, c0, k0);
    load_coef<V>(k + C, c0, k1);
  }
  for (int e = blockIdx.x * 256 + threadIdx.x; e < nvec; e += gridDim.x * 256) {
    const P pk = *reinterpret_cast<const P*>(x + (int64_t)e * V);
    P zk;
    if (z) zk = *reinterpret_cast<const P*>(z + (int64_t)e * V);
    P o;
    if (nhwc) {
      if (!hoist) {
        const int c0 = (e % CV) * V;
        load_coef<V>(k, c0, k0);
        load_coef<V>(k + C, c0, k1);
      }
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float v = to_f(pk.v[i]) * k0[i] + k1[i];
        if (z) v += to_f(zk.v[i]);
        if (relu) v = fmaxf(v, 0.f);
        o.v[i] = from_f<T>(v);
      }
    } else {
      const int c = (e / SV) % C;
      const float k0 = k[c], k1 = k[C + c];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float v = to_f(pk.v[i]) * k0 + k1;
        if (z) v += to_f(zk.v[i]);
        if (relu) v = fmaxf(v, 0.f);
        o.v[i] = from_f<T>(v);
      }
    }
    *reinterpret_cast<P*>(y + (int64_t)e * V) = o;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_reduce_nchw_vec(const T* __restrict__ dy, const T* __restrict__ x,
                                                             const T* __restrict__ ym, const float* __restrict__ mean,
                                                             float* __restrict__ part, int N, int C, int S) {
  constexpr int V = BnVec<T>::V;
  typedef typename BnVec<T>::P P;
  __shared__ float red[4];
  const int c = blockIdx.x;
  const int SV = S / V;
  const int total = N * SV;
  const int per = (total + gridDim.y - 1) / gridDim.y;
  const int e0 = blockIdx.y * per, e1 = min(e0 + per, total);
  const float mu = mean[c];
  float s1 = 0.f, s2 = 0.f;
  for (int e = e0 + threadIdx.x; e < e1; e += 256) {
    const int n = e / SV, sv = e - n * SV;
    const int64_t off = ((int64_t)n * C + c) * S + (int64_t)sv * V;
    const P d = *reinterpret_cast<const P*>(dy + off);
    const P xv = *reinterpret_cast<const P*>(x + off);
    P yv;
    if (ym) yv = *reinterpret_cast<const P*>(ym + off);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float g = ym && !(to_f(yv.v[k]) > 0.f) ? 0.f : to_f(d.v[k]);
      s1 += g;
      s2 += g * (to_f(xv.v[k]) - mu);
    }
  }
  s1 = block_sum(s1, red);
  s2 = block_sum(s2, red);
  if (threadIdx.x == 0) {
    part[((int64_t)c * gridDim.y + blockIdx.y) * 2] = s1;
    part[((int64_t)c * gridDim.y + blockIdx.y) * 2 + 1] = s2;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_reduce_nhwc_vec(const T* __restrict__ dy, const T* __restrict__ x,
                                                             const T* __restrict__ ym, const float* __restrict__ mean,
                                                             float* __restrict__ part, int64_t R, int C, int cvb,
                                                             int rpb) {
  constexpr int V = BnVec<T>::V;
  typedef typename BnVec<T>::P P;
  __shared__ float sm[256 * V * 2];
  const int CV = C / V;
  const int tc = threadIdx.x % cvb, tr = threadIdx.x / cvb;
  const int cv = blockIdx.x * cvb + tc;
  float s1[V], s2[V], mu[V];
#pragma unroll
  for (int k = 0; k < V; ++k) s1[k] = s2[k] = 0.f;
  if (tr < rpb && cv < CV) {
#pragma unroll
    for (int k = 0; k < V; ++k) mu[k] = mean[cv * V + k];
    const int64_t step = (int64_t)rpb * gridDim.y;
    for (int64_t r = (int64_t)blockIdx.y * rpb + tr; r < R; r += step) {
      const P d = *reinterpret_cast<const P*>(dy + r * C + (int64_t)cv * V);
      const P xv = *reinterpret_cast<const P*>(x + r * C + (int64_t)cv * V);
      P yv;
      if (ym) yv = *reinterpret_cast<const P*>(ym + r * C + (int64_t)cv * V);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float g = ym && !(to_f(yv.v[k]) > 0.f) ? 0.f : to_f(d.v[k]);
        s1[k] += g;
        s2[k] += g * (to_f(xv.v[k]) - mu[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    sm[threadIdx.x * V + k] = s1[k];
    sm[256 * V + threadIdx.x * V + k] = s2[k];
  }
  __syncthreads();
  if (tr == 0 && cv < CV) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float a = 0.f, bb = 0.f;
      for (int q = 0; q < rpb; ++q) {
        const int id = q * cvb + tc;
        a += sm[id * V + k];
        bb += sm[256 * V + id * V + k];
      }
      float* p = part + ((int64_t)(cv * V + k) * gridDim.y + blockIdx.y) * 2;
      p[0] = a;
      p[1] = bb;
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_elemt_vec(const T* __restrict__ dy, const T* __restrict__ x,
                                                       const float* __restrict__ k, const T* __restrict__ ym,
                                                       T* __restrict__ dz, T* __restrict__ dx, int nvec, int C, int S,
                                                       int nhwc) {
  constexpr int V = BnVec<T>::V;
  typedef typename BnVec<T>::P P;
  const int SV = S / V, CV = C / V;
  const bool hoist = nhwc && ((int64_t)gridDim.x * 256) % CV == 0;  // as in bn_elemt_vec
  float k0[V], k1[V], k2[V];
  if (hoist) {
    const int c0 = ((blockIdx.x * 256 + threadIdx.x) % CV) * V;
    load_coef<V>(k, c0, k0);
    load_coef<V>(k + C, c0, k1);
    load_coef<V>(k + 2 * C, c0, k2);
  }
  for (int e = blockIdx.x * 256 + threadIdx.x; e < nvec; e += gridDim.x * 256) {
    P d = *reinterpret_cast<const P*>(dy + (int64_t)e * V);
    const P xv = *reinterpret_cast<const P*>(x + (int64_t)e * V);
    if (ym) {  // fused ReLU: the gradient passes where the forward output was positive
      const P yv = *reinterpret_cast<const P*>(ym + (int64_t)e * V);
#pragma unroll
      for (int i = 0; i < V; ++i)
        if (!(to_f(yv.v[i]) > 0.f)) d.v[i] = from_f<T>(0.f);
      if (dz) *reinterpret_cast<P*>(dz + (int64_t)e * V) = d;  // the residual input's gradient
    }
    P o;
    if (nhwc) {
      if (!hoist) {
        const int c0 = (e % CV) * V;
        load_coef<V>(k, c0, k0);
        load_coef<V>(k + C, c0, k1);
        load_coef<V>(k + 2 * C, c0, k2);
      }
#pragma unroll
      for (int i = 0; i < V; ++i) o.v[i] = from_f<T>(to_f(d.v[i]) * k0[i] + to_f(xv.v[i]) * k1[i] + k2[i]);
    } else {
      const int c = (e / SV) % C;
      const float k0 = k[c], k1 = k[C + c], k2 = k[2 * C + c];
#pragma unroll
      for (int i = 0; i < V; ++i) o.v[i] = from_f<T>(to_f(d.v[i]) * k0 + to_f(xv.v[i]) * k1 + k2);
    }
    *reinterpret_cast<P*>(dx + (int64_t)e * V) = o;
  }
}

// parallel (sum_dy, sum_dy_xmu) finalize for many splits: one block per channel
__global__ void __launch_bounds__(256) bn_bwd_finalize_par_kernel(const float* __restrict__ part, int splits,
                                                                 float* __restrict__ sum_dy,
                                                                 float* __restrict__ sum_dy_xmu) {
  __shared__ float red[4];
  const int64_t c = blockIdx.x;
  float a = 0.f, b = 0.f;
  for (int k = threadIdx.x; k < splits; k += 256) {
    a += part[(c * splits + k) * 2];
    b += part[(c * splits + k) * 2 + 1];
  }
  a = block_sum(a, red);
  b = block_sum(b, red);
  if (threadIdx.x == 0) {
    sum_dy[c] = a;
    sum_dy_xmu[c] = b;
  }
}

// parallel combine of c-major local partials (groups >= 64): one block per channel
__global__ void __launch_bounds__(256) bn_combine_par_kernel(const float* __restrict__ in, int groups,
                                                            float* __restrict__ mean, float* __restrict__ var,
                                                            float* __restrict__ count, BnFinish fin) {
  __shared__ float sm[3][4];
  const int64_t c = blockIdx.x;
  Welford t{0.f, 0.f, 0.f};
  for (int g = threadIdx.x; g < groups; g += 256) {
    const float* p = in + (c * groups + g) * 3;
    t = wf_merge(t, Welford{p[0], p[1], p[2]});
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Welford b{__shfl_xor(t.mean, o, 64), __shfl_xor(t.m2, o, 64), __shfl_xor(t.n, o, 64)};
    t = wf_merge(t, b);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    sm[0][wid] = t.mean;
    sm[1][wid] = t.m2;
    sm[2][wid] = t.n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Welford r{sm[0][0], sm[1][0], sm[2][0]};
    for (int k = 1; k < 4; ++k) r = wf_merge(r, Welford{sm[0][k], sm[1][k], sm[2][k]});
    bn_finish(r, c, mean, var, count, fin);
  }
}

static inline int bn_vec(int dt) { return dt == kF32 ? 4 : 8; }

// NHWC block geometry: cvb channel vectors x rpb row lanes (cvb * rpb <= 256)
static inline void bn_nhwc_geom(int64_t C, int V, int& cvb, int& rpb, int& gx) {
  const int CV = (int)(C / V);
  cvb = CV < 64 ? CV : 64;
  rpb = 256 / cvb;
  gx = (CV + cvb - 1) / cvb;
}

static inline bool bn_vec_ok(const void* p, int64_t N, int64_t C, int64_t S, int nhwc, int V) {
  if (((uintptr_t)p & 15) || N * C * S / V >= (1ll << 31) || C >= (1 << 30)) return false;
  return nhwc ? (C % V == 0 && C / V <= 256 * 64) : (S % V == 0 && N * (S / V) < (1ll << 31));
}

static inline int bn_splits(int64_t N, int64_t S, int64_t C, int nhwc, int V) {
  if (nhwc) {
    // ~1024 blocks over the channel-vector groups, >= 8 rows per row lane (2048 blocks / a 2048
    // split cap measured slower: bwd reduce 59 -> 64 us average on ResNet-50)
    int cvb, rpb, gx;
    bn_nhwc_geom(C, V, cvb, rpb, gx);
    const int64_t R = N * S;
    int64_t sp = (1024 + gx - 1) / gx;
    const int64_t cap = R / (8 * (int64_t)rpb);
    if (sp > cap) sp = cap;
    if (sp < 1) sp = 1;
    if (sp > 512) sp = 512;
    return (int)sp;
  }
  // enough blocks to fill the chip: ~2048 blocks total, each >= 1024 elements
  int64_t per_c = (N * S + 1023) / 1024;
  int64_t want = (2048 + C - 1) / C;
  int64_t sp = per_c < want ? per_c : want;
  if (sp < 1) sp = 1;
  if (sp > 256) sp = 256;
  return (int)sp;
}

int bn_splits_for(int64_t N, int64_t C, int64_t S, int nhwc, int dt) {
  return bn_splits(N, S, C, nhwc, bn_vec(dt));
}

int bn_stats(const void* x, float* part, int64_t N, int64_t C, int64_t S, int nhwc, int dt, int* splits_out,
             hipStream_t s) {
  const int V = bn_vec(dt);
  const int sp = bn_splits(N, S, C, nhwc, V);
  *splits_out = sp;
  if (C == 0) return 0;
  if (bn_vec_ok(x, N, C, S, nhwc, V)) {
    if (nhwc) {
      int cvb, rpb, gx;
      bn_nhwc_geom(C, V, cvb, rpb, gx);
      APEX_DISPATCH_T(dt, T,
          hipLaunchKernelGGL((bn_stats_nhwc_vec<T>), dim3(gx, sp), dim3(256), 0, s, (const T*)x, part, N * S,
                             (int)C, cvb, rpb));
    } else {
      APEX_DISPATCH_T(dt, T,
          hipLaunchKernelGGL((bn_stats_nchw_vec<T>), dim3((unsigned)C, sp), dim3(256), 0, s, (const T*)x, part,
                             (int)N, (int)C, (int)S));
    }
  } else {
    APEX_DISPATCH_T(dt, T,
        hipLaunchKernelGGL((bn_stats_kernel<T>), dim3((unsigned)C, sp), dim3(256), 0, s, (const T*)x, part, N, C,
                           S, nhwc));
  }
  return (int)hipGetLastError();
}

int bn_combine(const float* in, int groups, int64_t C, int gmajor, float* mean, float* var, float* count,
               hipStream_t s, float* invstd, float eps, float* rmean, float* rvar, float momentum,
               float* triple, int64_t* ntrack) {
  if (C == 0) return 0;
  const BnFinish fin{invstd, rmean, rvar, triple, ntrack, eps, momentum};
  if (!gmajor && groups >= 64) {
    hipLaunchKernelGGL(bn_combine_par_kernel, dim3((unsigned)C), dim3(256), 0, s, in, groups, mean, var, count, fin);
  } else {
    hipLaunchKernelGGL(bn_combine_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, in, groups, C,
                       gmajor, mean, var, count, fin);
  }
  return (int)hipGetLastError();
}

int bn_elemt(const void* x, const float* mean, const float* invstd, const void* w, const void* b, const void* z,
             void* y, int64_t N, int64_t C, int64_t S, int nhwc, int relu, int dt, int wdt, float* coef,
             hipStream_t s) {
  const int64_t total = N * C * S;
  if (total == 0) return 0;
  if (!w && !b) wdt = kF32;
  const int V = bn_vec(dt);
  if (coef && bn_vec_ok(x, N, C, S, nhwc, V) && ((uintptr_t)y & 15) == 0 && ((uintptr_t)coef & 15) == 0 &&
      ((uintptr_t)z & 15) == 0) {
    APEX_DISPATCH_T(wdt, W,
        hipLaunchKernelGGL((bn_coef_fwd_kernel<W>), dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, mean, invstd,
                           (const W*)w, (const W*)b, coef, (int)C));
    const int64_t nvec = total / V;
    const int64_t grid = min((nvec + 255) / 256, (int64_t)4096);
    APEX_DISPATCH_T(dt, T,
        hipLaunchKernelGGL((bn_elemt_vec<T>), dim3((unsigned)grid), dim3(256), 0, s, (const T*)x, coef, (const T*)z,
                           (T*)y, (int)nvec, (int)C, (int)S, nhwc, relu));
    return (int)hipGetLastError();
  }
  const int64_t grid = min((total + 255) / 256, (int64_t)8192);
  APEX_DISPATCH_T(dt, T, APEX_DISPATCH_T(wdt, W,
      hipLaunchKernelGGL((bn_elemt_kernel<T, W>), dim3((unsigned)grid), dim3(256), 0, s, (const T*)x, mean,
                         invstd, (const W*)w, (const W*)b, (const T*)z, (T*)y, N, C, S, nhwc, relu)));
  return (int)hipGetLastError();
}

int bn_bwd_reduce(const void* dy, const void* x, const void* ym, const float* mean, float* part, float* sum_dy,
                  float* sum_dy_xmu, int64_t N, int64_t C, int64_t S, int nhwc, int dt, hipStream_t s) {
  if (C == 0) return 0;
  const int V = bn_vec(dt);
  const int sp = bn_splits(N, S, C, nhwc, V);
  if (bn_vec_ok(x, N, C, S, nhwc, V) && ((uintptr_t)dy & 15) == 0 && ((uintptr_t)ym & 15) == 0) {
    if (nhwc) {
      int cvb, rpb, gx;
      bn_nhwc_geom(C, V, cvb, rpb, gx);
      APEX_DISPATCH_T(dt, T,
          hipLaunchKernelGGL((bn_bwd_reduce_nhwc_vec<T>), dim3(gx, sp), dim3(256), 0, s, (const T*)dy,
                             (const T*)x, (const T*)ym, mean, part, N * S, (int)C, cvb, rpb));
    } else {
      APEX_DISPATCH_T(dt, T,
          hipLaunchKernelGGL((bn_bwd_reduce_nchw_vec<T>), dim3((unsigned)C, sp), dim3(256), 0, s, (const T*)dy,
                             (const T*)x, (const T*)ym, mean, part, (int)N, (int)C, (int)S));
    }
  } else {
    APEX_DISPATCH_T(dt, T,
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<T>), dim3((unsigned)C, sp), dim3(256), 0, s, (const T*)dy,
                           (const T*)x, (const T*)ym, mean, part, N, C, S, nhwc));
  }
  if (sp >= 64)
    hipLaunchKernelGGL(bn_bwd_finalize_par_kernel, dim3((unsigned)C), dim3(256), 0, s, part, sp, sum_dy, sum_dy_xmu);
  else
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, part, sp, C,
                       sum_dy, sum_dy_xmu);
  return (int)hipGetLastError();
}

int bn_bwd_elemt(const void* dy, const void* x, const float* mean, const float* invstd, const void* w,
                 const float* sum_dy, const float* sum_dy_xmu, const float* count, const void* ym, void* dz,
                 void* dx, int64_t N, int64_t C, int64_t S, int nhwc, int dt, int wdt, float* coef, hipStream_t s) {
  const int64_t total = N * C * S;
  if (total == 0) return 0;
  if (!w) wdt = kF32;
  const int V = bn_vec(dt);
  if (coef && bn_vec_ok(x, N, C, S, nhwc, V) && ((uintptr_t)dy & 15) == 0 && ((uintptr_t)dx & 15) == 0 &&
      ((uintptr_t)coef & 15) == 0 && ((uintptr_t)ym & 15) == 0 && ((uintptr_t)dz & 15) == 0) {
    APEX_DISPATCH_T(wdt, W,
        hipLaunchKernelGGL((bn_coef_bwd_kernel<W>), dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, mean, invstd,
                           (const W*)w, sum_dy, sum_dy_xmu, count, coef, (int)C));
    const int64_t nvec = total / V;
    const int64_t grid = min((nvec + 255) / 256, (int64_t)4096);
    APEX_DISPATCH_T(dt, T,
        hipLaunchKernelGGL((bn_bwd_elemt_vec<T>), dim3((unsigned)grid), dim3(256), 0, s, (const T*)dy, (const T*)x,
                           coef, (const T*)ym, (T*)dz, (T*)dx, (int)nvec, (int)C, (int)S, nhwc));
    return (int)hipGetLastError();
  }
  const int64_t grid = min((total + 255) / 256, (int64_t)8192);
  APEX_DISPATCH_T(dt, T, APEX_DISPATCH_T(wdt, W,
      hipLaunchKernelGGL((bn_bwd_elemt_kernel<T, W>), dim3((unsigned)grid), dim3(256), 0, s, (const T*)dy,
                         (const T*)x, mean, invstd, (const W*)w, sum_dy, sum_dy_xmu, count, (const T*)ym,
                         (T*)dz, (T*)dx, N, C, S, nhwc)));
  return (int)hipGetLastError();
}

}  // namespace apex
