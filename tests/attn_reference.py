"""Float64 reference of flash attention (csrc/attention_common.h, attention_fwd.h, attention_bwd.h,
attention_impl.h, attention_f32.hip, attention_gqa.hip), the per-element error bound its outputs are
held to, an independent NumPy dropout keep mask, an fp32 CPU emulation of the kernels' arithmetic with
its mutants, and the shared test cases.

A plain helper module in the style of gemm_reference.py: no tests, no fixtures, and it never calls the
extension. tests/test_attn_reference.py (emulation and mutants against this reference, on the CPU) and
tests/test_attn_numerics_gpu.py (the HIP kernels against it) share the case tables and the seeded
generators below.

Reference (reference()). The API's semantics per (batch, head), operands at their stored values
converted to double: a = q.k * scale + bias, causal mask key > query (top-left aligned for Sq != Sk),
key lengths per batch, K/V head h // group for grouped-query attention; P = softmax(a) over the visible
keys, W = P * keep * r with r = 256 / (256 - thresh); O = W V, lse = log sum exp(a). A row with no visible
key has O = 0, lse = +inf and zero gradients. Backward, as flash_attn_bwd defines it — a function of
(q, k, v, o, lse, dO), not of (q, k, v, dO) alone: P' = exp(a - lse) from the lse the forward STORED,
delta = sum_d dO * o from the o it STORED (both kernels read these two tensors, they recompute neither),
dS = P' (dP keep r - delta), dV = W'^T dO, dK = scale dS^T Q, dQ = scale dS K, dbias = dS summed over the
bias's broadcast dims; grouped K/V heads sum dK / dV over their group. Taking the stored o and lse is what
makes the dQ / dK bound tight: the error of O does not enter delta, only its accumulation does. (That the
stored o and lse are right is the forward's own check.) dsum is checked against the float64 column sums
of the dq / dk / dv the kernel stored, as the GEMM bias gradient is.

The bound, per element, with u = HALF_ULP[T], uP = u for the 16-bit units and 0 for the fp32 unit (which
never rounds to 16 bits), E24 = 2**-24 (one fp32 rounding), E23 = 2**-23, EACC = one MFMA addition (E23 for
the 16-bit MFMA, which may truncate; E24 for the f32 MFMA, an fmaf chain), tile = 64 keys (32 in the fp32
unit), nt = tiles of the key range. Every count of additions is the count of NONZERO terms (adding an exact
zero is exact): nnz(x, y) = additions of nonzero products in x . y. eps(c) = the relative error of the fp32
constant the kernel holds for c, computed, not assumed (f32_const_error). Derived from the code, not tuned:
  scores      ds = (nnz EACC [+ 2 E24 in fp32: scale * q and the product]) |q|.|k|; products of 16-bit values
              are exact in fp32.
  exp2 arg    eta = scale log2e ds + eps_c (|qk2| + |b2|) + E24 (|a2 - m2| [+ |a2| with a bias]) + 4 (nt - 1) E24 M2:
              a2 = a log2e, qk2 and b2 its q.k and bias parts, m2 the row max, M2 = max |a2| of the row,
              eps_c = eps(scale log2e) + eps(scale) + eps(log2e). x = fma(s, sl2, -m sl2) rounds once, relative to
              x itself; the shift m sl2 cancels between p and l except where alpha = exp2((m_old - m_new) sl2)
              rounds it again, once per further tile; with a bias fma(s, scale, bias) (or s + bias) rounds once more.
  P           rho = ln2 eta + nt E23: bare v_exp_f32 is within one ulp (E23), alpha's once per tile.
  row sum     rho_l = sum_k P rho + (nvis + 2 nt - 2) E24: nvis - 1 additions of the visible keys' p plus the
              cross-half add, l * alpha + psum from the second tile on (l is summed from the UNROUNDED p).
  O           u |O| + TINY + sum_k W (uP + rho) |V| + (rho_l + 2 E24 [+ E24: drop_scale]) sum_k W |V|
              + (nnz(W, V) + nt - 1) EACC sum_k W |V| + P_TINY r sum_{kept visible k} |V|: P is rounded to T for the
              PV product (uP), inv = 1 / l and the multiply, the MFMA additions and the alpha rescale per tile;
              P_TINY: an unnormalised p <= 1 that is subnormal in fp16 rounds with an absolute error (2**-24),
              and v_exp_f32 flushes below 2**-126.
  lse         rho_l + E24 (ln2 |m2| + 2 |lse|) + eps(ln2) |lse| + 2 E23 ln2 |log2 l|: m * sl2 + log2f(l) may be
              contracted (ln2 |m2|), the add, the multiply by kLn2; log2f within an ulp of its result.
  backward P' eta' = scale log2e ds + eps_c (|qk2| + |b2|) + E24 (|lse2| [16-bit: lse * log2e rounded when staged]
              + 2 |a2 - lse2| [+ |a2| + |b2| + |lse2| with a bias]), rho' = ln2 eta' + E23.
  dP          ddp = (nnz EACC [+ E24 in fp32]) |dO|.|V|.
  delta       against the float64 sum over the stored o: (nnz - 1 [nnz in fp32]) E24 sum_d |dO o|.
  dS (fp32)   e_dS = |dS| (rho' + 2 E24 [+ E24: drop_scale]) + P' (r keep ddp + e_delta [+ E24 r keep |dP|]): the
              subtraction (or FMA) and the multiply by P'. This is the dbias bound (plus n E24 sum |dS| for the n
              nonzero terms added into a slot).
  dS in T     e_dS + uP |dS| + TINY: the operand of the dK / dQ products.
  dV          us |dV| + TINY + sum_q W' (uP + rho') |dO| + P_TINY r sum_q keep |dO| + (nnz EACC + epi) sum_q W' |dO|,
              us = u on a 16-bit store and 0 in the fp32 unit (whose last rounding is the epilogue multiply),
              epi = E24 + eps(scale) [+ E24 with dropout].
  dK          us |dK| + TINY + scale sum_q e_dS,T |Q| + scale (nnz EACC + epi) sum_q |dS| |Q|.
  dQ          the same over keys with |K|.
  grouped     dK = sum over the group of the stored per-head dK: the per-head bounds add, plus
              g E24 sum_g |dK_h| (one fp32 sum) and u |dK| + TINY (one rounding); dV alike.
  dsum        E24 times the sum, over the additions of the kernels' own summation order (emu_dsum), of the
              sum of |x| below each addition.
  TINY        max(TINY[T], 2**-126): the f32 MFMA accumulators and v_exp_f32 flush results below 2**-126 to zero, so
              a bf16 or fp32 result, and a dS on its way into a product, has that absolute error, not the
              subnormal spacing. (Found on the GPU: an fp32 dK of 1.6e-39 came back as 0.)
None of these was fitted to a GPU run.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np
import torch

from mt_reference import BF16, DT_NAME, F16, F32, HALF_ULP, TINY  # noqa: F401

DTYPES = [BF16, F16, F32]
INF = float("inf")
E23, E24 = 2.0 ** -23, 2.0 ** -24
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
FWD_TILE = {BF16: 64, F16: 64, F32: 32}      # keys per forward tile (kFwdKB, kF32Tile)
BWD_BK = 128                                # keys per backward workgroup; fused backward for Sk <= BWD_BK
P_TINY = {BF16: 2.0 ** -126, F16: 2.0 ** -24, F32: 2.0 ** -126}
FTZ32 = 2.0 ** -126                         # fp32 results below it are flushed to zero (MFMA, v_exp_f32)


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def drop_thresh(p: float) -> int:
    """kernels.h attn_drop_thresh: the 8-bit keep threshold of a dropout probability (0 = off)."""
    if p <= 0.0:
        return 0
    return min(255, max(1, int(p * 256.0 + 0.5)))


# ----------------------------------------------------------------------------
# dropout keep mask, NumPy (independent of the extension and of the scalar Python version)
# ----------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def _philox4x32_7(seed, subseq, offset):
    """Philox4x32-7 on uint64 arrays `subseq`, `offset` (one call per element): four uint64 arrays < 2**32."""
    s = np.uint64(32)
    key0 = np.uint64(seed & 0xFFFFFFFF)
    key1 = np.uint64((seed >> 32) & 0xFFFFFFFF)
    c0, c1, c2, c3 = offset & _M32, offset >> s, subseq & _M32, subseq >> s
    for _ in range(7):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ key0, p1 & _M32, (p0 >> s) ^ c3 ^ key1, p0 & _M32
        key0 = (key0 + np.uint64(0x9E3779B9)) & _M32
        key1 = (key1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def keep_mask(seed, offset, BH, Sq, Sk, thresh):
    """bool [BH, Sq, Sk]: the keep flag of every (row, key), by the mapping documented above DropStream
    (attention_common.h): one stream per (row, half hl = bit 2 of the key): a Philox4x32-7 call (counter
    offset + hl, subsequence bh * Sq + row) seeds xorshift128; every 32-key block takes the stream's next
    four words; key k of a block <-> byte k >> 3 of word k & 3 of half (k >> 2) & 1; kept iff byte >= thresh."""
    nblk = (Sk + 31) // 32
    rows = np.arange(BH * Sq, dtype=np.uint64)
    words = np.empty((2, BH * Sq, 4 * nblk), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for hl in (0, 1):
            off = np.full_like(rows, (offset + hl) & 0xFFFFFFFFFFFFFFFF)
            x, y, z, w = _philox4x32_7(seed, rows, off)
            w = w | ((x | y | z | w) == 0).astype(np.uint64)
            for i in range(4 * nblk):
                t = (x ^ (x << np.uint64(11))) & _M32
                x, y, z = y, z, w
                w = (w ^ (w >> np.uint64(19)) ^ t ^ (t >> np.uint64(8))) & _M32
                words[hl, :, i] = w
    key = np.arange(nblk * 32)
    k = key % 32
    sel = words[(k >> 2) & 1, :, 4 * (key // 32) + (k & 3)]          # [keys, rows]
    byte = (sel >> (8 * (k >> 3)).astype(np.uint64)[:, None]) & np.uint64(0xFF)
    return (byte >= np.uint64(thresh)).T[:, :Sk].reshape(BH, Sq, Sk)


# ----------------------------------------------------------------------------
# operands of one call
# ----------------------------------------------------------------------------
@dataclass
class Ops:
    """One attention call, API layout: q, do [B, Sq, H, D]; k, v [B, Sk, Hk, D]; bias [B|1, H|1, Sq|1, Sk] or
    None; k_lens a tuple of B ints or None; keep a bool [B, H, Sq, Sk] tensor or None (with thresh)."""
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    do: torch.Tensor
    scale: float
    causal: bool = False
    k_lens: tuple | None = None
    bias: torch.Tensor | None = None
    keep: torch.Tensor | None = None
    thresh: int = 0

    @property
    def dims(self):
        B, Sq, H, D = self.q.shape
        return B, H, self.k.shape[2], Sq, self.k.shape[1], D

    @property
    def r(self):
        return 256.0 / (256.0 - self.thresh) if self.thresh else 1.0


def bh(t):
    """[B, S, H, D] (API layout) -> [B, H, S, D]."""
    return t.permute(0, 2, 1, 3)


def visible(ops, mut=None):
    """bool [B, 1, Sq, Sk]: key visible to the query under the causal mask and the key lengths."""
    B, H, Hk, Sq, Sk, D = ops.dims
    key, qi = torch.arange(Sk)[None, :], torch.arange(Sq)[:, None]
    vis = torch.ones(B, 1, Sq, Sk, dtype=torch.bool)
    if ops.causal:
        shift = {"causal_plus1": 1, "causal_minus1": -1}.get(mut, 0)
        vis = vis & (key <= qi + shift)
    if ops.k_lens is not None:
        kl = torch.tensor(ops.k_lens)
        if mut == "klens_wrong_batch":
            kl = kl.roll(1)
        vis = vis & (key[None, None] < kl[:, None, None, None])
    if mut == "drop_last_ragged_key" and Sk % 64:
        vis = vis & (key != Sk - 1)
    return vis


def _kv_bh(t, H, mut=None):
    """K or V [B, Sk, Hk, D] -> float64 [B, H, Sk, D], head h reading K/V head h // group."""
    Hk = t.shape[2]
    idx = torch.arange(H) % Hk if mut == "kv_head_mod" else torch.arange(H) // (H // Hk)
    return bh(t.double())[:, idx]


def reference(ops, o_stored=None, lse_stored=None):
    """Float64 forward and backward (module docstring). o_stored [B, Sq, H, D] and lse_stored [B, H, Sq]: what
    the forward under test stored; None: the reference's own O and lse. Every result in [B, H, S, D] /
    [B, H, Sq, Sk] layout; dK, dV [B, Hk, Sk, D] with their per-query-head parts dKx, dVx."""
    B, H, Hk, Sq, Sk, D = ops.dims
    q, do = bh(ops.q.double()), bh(ops.do.double())
    k, v = _kv_bh(ops.k, H), _kv_bh(ops.v, H)
    sqk = q @ k.transpose(-1, -2) * ops.scale
    bias = None if ops.bias is None else ops.bias.double()
    a = sqk if bias is None else sqk + bias
    vis = visible(ops) & (a > -INF)
    am = torch.where(vis, a, torch.full_like(a, -INF))
    m = am.max(-1, keepdim=True).values if Sk else torch.full((B, H, Sq, 1), -INF, dtype=torch.float64)
    live = m > -INF
    ms = torch.where(live, m, torch.zeros_like(m))
    e = torch.exp(am - ms)
    l = e.sum(-1, keepdim=True)
    P = torch.where(live, e / l.clamp(min=1e-300), torch.zeros_like(e))
    lse = torch.where(live, ms + torch.log(l.clamp(min=1e-300)), torch.full_like(ms, INF)).squeeze(-1)
    keep = torch.ones_like(P) if ops.keep is None else ops.keep.double()
    r = ops.r
    W = P * keep * r
    O = W @ v
    # backward from the stored o and lse
    ob = O if o_stored is None else bh(o_stored.double())
    lb = lse if lse_stored is None else lse_stored.double()
    lbs = torch.where(lb < INF, lb, torch.zeros_like(lb))[..., None]
    Pb = torch.where(vis & (lb < INF)[..., None], torch.exp(am - lbs), torch.zeros_like(am))
    Wb = Pb * keep * r
    dP = do @ v.transpose(-1, -2)
    delta = (do * ob).sum(-1, keepdim=True)
    dS = Pb * (dP * keep * r - delta)
    dVx = Wb.transpose(-1, -2) @ do
    dKx = dS.transpose(-1, -2) @ q * ops.scale
    dQ = dS @ k * ops.scale
    g = H // Hk
    dK, dV = dKx.view(B, Hk, g, Sk, D).sum(2), dVx.view(B, Hk, g, Sk, D).sum(2)
    dbias = None if bias is None else reduce_to(dS, bias.shape)
    return SimpleNamespace(O=O, lse=lse, dQ=dQ, dK=dK, dV=dV, dKx=dKx, dVx=dVx, dbias=dbias, P=P, W=W, Pb=Pb, Wb=Wb,
                           dS=dS, dP=dP, delta=delta, a=a, sqk=sqk, vis=vis, m=ms, live=live, l=l, lse_b=lb, o_b=ob,
                           keep=keep, q=q, k=k, v=v, do=do, bias=bias)


def f32_const_error(x):
    """Relative error of the fp32 constant the kernels hold for x (at most 2**-24, usually well below)."""
    return abs(float(torch.tensor(float(x), dtype=torch.float32)) / float(x) - 1.0)


def reduce_to(x, shape):
    """Sum a [B, H, Sq, Sk] tensor over the dims in which `shape` is 1."""
    dims = [i for i in range(3) if shape[i] == 1 and x.shape[i] != 1]
    return x.sum(dims, keepdim=True) if dims else x


def bounds(R, ops, T, stored=True):
    """{name: bound} for O, lse, dQ, dK, dV, dbias (module docstring). stored = True: R's backward was formed from
    the stored o and lse; "o": from the stored o and the reference's own lse (a caller that never sees lse), so the
    error of lse enters P'; False: from neither, so the error of O enters delta as well."""
    B, H, Hk, Sq, Sk, D = ops.dims
    u, tiny = HALF_ULP[T], max(TINY[T], FTZ32)
    f32 = T == F32
    uP, tinyP = (0.0 if f32 else u), tiny
    nt = max(1, -(-Sk // FWD_TILE[T]))
    r, scale = ops.r, abs(ops.scale)
    qa, ka, va, doa = R.q.abs(), R.k.abs(), R.v.abs(), R.do.abs()
    nz = lambda t: (t != 0).double()  # noqa: E731
    kT = lambda t: t.transpose(-1, -2)  # noqa: E731
    visd = R.vis.double()
    EACC = E24 if f32 else E23       # one MFMA addition: the f32 MFMA is an fmaf chain, the 16-bit one may truncate
    nnz = lambda x, y: (nz(x) @ nz(y) - 1).clamp(min=0)  # noqa: E731  additions of nonzero products
    ds = (nnz(R.q, kT(R.k)) * EACC + (2 * E24 if f32 else 0.0)) * (qa @ kT(ka))
    fin = lambda t: torch.where(R.vis, t, torch.zeros_like(t))  # noqa: E731
    has_bias = R.bias is not None
    a2 = fin(R.a).abs() * LOG2E
    aqk2 = fin(R.sqk).abs() * LOG2E
    b2 = torch.zeros_like(a2) if not has_bias else fin(R.bias.expand_as(R.a)).abs() * LOG2E
    m2 = R.m * LOG2E
    M2 = a2.max(-1, keepdim=True).values if Sk else torch.zeros_like(m2)
    eps_c = f32_const_error(ops.scale * LOG2E) + f32_const_error(ops.scale) + f32_const_error(LOG2E)
    nvis = visd.sum(-1, keepdim=True)
    eta = (scale * LOG2E * ds + eps_c * (aqk2 + b2)
           + E24 * (fin(R.a * LOG2E - m2).abs() + (a2 if has_bias else 0.0) + 4 * (nt - 1) * M2))
    rho = (LN2 * eta + nt * E23) * visd
    rho_l = (R.P * rho).sum(-1, keepdim=True) + (nvis + 2 * nt - 2).clamp(min=0) * E24
    keepvis = visd * R.keep
    out = {}
    out["O"] = (u * R.O.abs() + tiny + (R.W * (uP + rho)) @ va
                + (R.W @ va) * (rho_l + (3 if ops.thresh else 2) * E24) + (nnz(R.W, R.v) + nt - 1) * EACC * (R.W @ va)
                + P_TINY[T] * r * (keepvis @ va))
    log2l = torch.where(R.live, torch.log2(R.l.clamp(min=1e-300)), torch.zeros_like(R.l)).abs()
    lse_f = torch.where(R.live, R.lse[..., None], torch.zeros_like(R.m)).abs()
    e_lse = (rho_l + E24 * (LN2 * m2.abs() + 2 * lse_f) + f32_const_error(LN2) * lse_f + 2 * E23 * LN2 * log2l
             + FTZ32).squeeze(-1)
    out["lse"] = e_lse
    # backward
    lb = torch.where(R.lse_b < INF, R.lse_b, torch.zeros_like(R.lse_b))[..., None]
    l2 = lb.abs() * LOG2E
    eta_b = (scale * LOG2E * ds + eps_c * (aqk2 + b2)
             + E24 * ((0.0 if f32 else l2) + 2 * fin(R.a * LOG2E - lb * LOG2E).abs()
                      + ((a2 + b2 + l2) if has_bias else 0.0)))
    rho_b = (LN2 * eta_b + E23) * visd
    e_delta = ((nz(R.do * R.o_b).sum(-1, keepdim=True) - (0 if f32 else 1)).clamp(min=0) * E24
               * (doa * R.o_b.abs()).sum(-1, keepdim=True))
    if stored != True:  # noqa: E712  ("o": delta from the stored o, P' from the reference's lse; False: neither)
        rho_b = rho_b + e_lse[..., None] * visd
        if stored is False:
            e_delta = e_delta + (doa * out["O"]).sum(-1, keepdim=True)
    drop = 1.0 if ops.thresh else 0.0
    epi = E24 + f32_const_error(ops.scale) + drop * E24     # the epilogue multiply and its constant
    ddp = (nnz(R.do, kT(R.v)) * EACC + (E24 if f32 else 0.0)) * (doa @ kT(va))
    dSa = R.dS.abs()
    e_dS = dSa * (rho_b + (2 + drop) * E24) + R.Pb * (r * R.keep * ddp + e_delta + drop * E24 * r * R.keep * R.dP.abs())
    e_dST = e_dS + uP * dSa + tinyP * visd
    us = 0.0 if f32 else u            # rounding on store: the fp32 unit's last rounding is the epilogue multiply
    e_dVx = (us * R.dVx.abs() + tiny + kT(R.Wb * (uP + rho_b)) @ doa + P_TINY[T] * r * (kT(keepvis) @ doa)
             + (kT(R.Wb) @ doa) * (nnz(kT(R.Wb), R.do) * EACC + epi))
    e_dKx = (us * R.dKx.abs() + tiny + scale * (kT(e_dST) @ qa)
             + scale * (kT(dSa) @ qa) * (nnz(kT(R.dS), R.q) * EACC + epi))
    out["dQ"] = (us * R.dQ.abs() + tiny + scale * (e_dST @ ka)
                 + scale * (dSa @ ka) * (nnz(R.dS, R.k) * EACC + epi))
    g = H // Hk
    if g == 1:
        out["dK"], out["dV"] = e_dKx, e_dVx
    else:
        grp = lambda t: t.view(B, Hk, g, Sk, D).sum(2)  # noqa: E731
        out["dK"] = grp(e_dKx) + g * E24 * grp(R.dKx.abs()) + u * R.dK.abs() + tiny
        out["dV"] = grp(e_dVx) + g * E24 * grp(R.dVx.abs()) + u * R.dV.abs() + tiny
    if has_bias:   # n: the nonzero terms added into a slot (adding an exact zero is exact)
        n = reduce_to(nz(R.dS), R.bias.shape)
        out["dbias"] = reduce_to(e_dS, R.bias.shape) + n * E24 * reduce_to(dSa, R.bias.shape) + FTZ32
    return out


def dsum_depth(S):
    """Additions one stored element passes through on its way into a dsum slot, (dq, dk / dv). dK / dV (emit in
    attn_bwd_kernel): 16 sequential per lane, the lane ^ 32 partner, three adds over the four waves, one atomic
    per 128-key block. dQ: the fused kernel adds a lane's query once per 32-query step, then group_sum<16> (4)
    and the two query-tile waves' atomics; the dQ kernel group_sum<32> (5) and one atomic per 32-query wave."""
    return -(-S // 32) + 6, 16 + 1 + 3 + -(-S // BWD_BK)


def dsum_expected(dq, dk, dv):
    """(ref, bound) [B, 3, H, D] of the packed-QKV bias-gradient partials from the dq / dk / dv the kernel stored
    ([B, S, H, D] each): float64 column sums over the positions. Bound: every fp32 addition of the kernels' own
    summation order (emu_dsum) is off by at most E24 times its result, which the sum of |x| below it bounds; the
    additions that meet in atomics (any order) are charged the whole slot's sum of |x| each."""
    x = torch.stack([t.detach().double() for t in (dq, dk, dv)], 1)          # [B, 3, S, H, D]
    return x.sum(2), E24 * emu_dsum(dq, dk, dv, count=True) + TINY[F32]


class _Abs:
    """|x| sums in float64 with the accumulated rounding budget: (a + b).cost = a.cost + b.cost + |a| + |b|
    (in units of E24) — what emu_dsum's additions may lose, on the same code path as the fp32 sums."""

    def __init__(self, val, cost=None):
        self.val, self.cost = val, torch.zeros_like(val) if cost is None else cost

    def __add__(self, o):
        v = self.val + o.val
        both = ((self.val != 0) & (o.val != 0)).double()      # adding an exact zero is exact
        return _Abs(v, self.cost + o.cost + both * v)

    def __getitem__(self, i):
        return _Abs(self.val[i], self.cost[i])

    def apply(self, f):
        return _Abs(f(self.val), f(self.cost))

    shape = property(lambda self: self.val.shape)


def _ap(x, f):
    return x.apply(f) if isinstance(x, _Abs) else f(x)


def _tree(x):
    """Butterfly sum over the last dim (a power of two). The rounding budget does not depend on which lanes the
    DPP steps pair: every level is charged the whole group's sum of |x|, for at most nnz - 1 levels."""
    if isinstance(x, _Abs):
        total, levels = x.val.sum(-1), math.log2(x.shape[-1])
        inexact = ((x.val != 0).sum(-1) - 1).clamp(min=0, max=levels).double()
        return _Abs(total, x.cost.sum(-1) + inexact * total)
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _seq(x, dim):
    """Sequential sum along dim."""
    acc = _ap(x, lambda t: t.select(dim, 0))
    for i in range(1, x.shape[dim]):
        acc = acc + _ap(x, lambda t: t.select(dim, i))
    return acc


def _atomic(x, dim):
    """Sum along dim of terms that meet in fp32 atomics, in any order: each of the nnz - 1 additions is charged the
    whole sum of |x|."""
    if isinstance(x, _Abs):
        total = x.val.sum(dim)
        return _Abs(total, x.cost.sum(dim) + ((x.val != 0).sum(dim) - 1).clamp(min=0).double() * total)
    return _seq(x, dim)


def emu_dsum(dq, dk, dv, count=False):
    """The kernels' order of the column sums of stored [B, S, H, D] gradients -> [B, 3, H, D]: in fp32, or
    (count) the rounding budget of that order in units of E24 (float64, from |x|). dK / dV (emit in
    attn_bwd_kernel): 16 sequential per lane, the lane ^ 32 partner, three adds over the four waves, one atomic
    per 128-key block. dQ: the fused kernel adds a lane's query once per 32-query step, then group_sum<16> and the
    two query-tile waves' atomics; the dQ kernel group_sum<32> and one atomic per 32-query wave."""
    B, S, H, D = dq.shape
    conv = (lambda t: _Abs(t.double().abs())) if count else (lambda t: t.float())
    pad = lambda t, m: torch.nn.functional.pad(t, (0, 0, 0, 0, 0, (-S) % m))  # noqa: E731
    outs = []
    x = conv(pad(dq, 32).view(B, -1, 32, H, D))             # [B, steps, 32 queries, H, D]
    if S <= BWD_BK:   # fused
        acc = _ap(_seq(x, 1), lambda t: t.view(B, 2, 16, H, D).permute(0, 1, 3, 4, 2))
        t = _tree(acc)
        outs.append(_ap(t, lambda z: z[:, 0]) + _ap(t, lambda z: z[:, 1]))
    else:             # dQ kernel
        outs.append(_atomic(_tree(_ap(x, lambda t: t.permute(0, 1, 3, 4, 2))), 1))
    for g in (dk, dv):                                      # key = 128 blk + 32 w + 8 g4 + 4 hl + e
        x = conv(pad(g, BWD_BK).view(B, -1, 4, 4, 2, 4, H, D).permute(0, 1, 2, 4, 3, 5, 6, 7))
        nb = x.shape[1]
        lane = _seq(_ap(x, lambda t: t.reshape(B, nb, 4, 2, 16, H, D)), 4)
        wave = _ap(lane, lambda t: t[:, :, :, 0]) + _ap(lane, lambda t: t[:, :, :, 1])
        w = [_ap(wave, lambda t, i=i: t[:, :, i]) for i in range(4)]
        outs.append(_atomic(((w[0] + w[1]) + w[2]) + w[3], 1))
    if count:
        return torch.stack([o.cost for o in outs], 1)
    return torch.stack(outs, 1)


# ----------------------------------------------------------------------------
# comparison
# ----------------------------------------------------------------------------
WORST = {}   # tag -> (largest ratio seen by check, case)


def ratio(got, ref, bound):
    """Worst |got - ref| / bound; 0 where got == ref (equal infinities included), inf where not finite."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if not got.numel():
        return 0.0, ()
    rr = (got - ref).abs() / bound
    rr = torch.where(got == ref, torch.zeros_like(rr), rr)
    rr = torch.where(torch.isfinite(rr), rr, torch.full_like(rr, INF))
    i = int(rr.argmax())
    return float(rr.reshape(-1)[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), rr.shape))


def check(got, ref, bound, what="", tag=None):
    worst, idx = ratio(got, ref, bound)
    if tag is not None and worst > WORST.get(tag, (-1.0, ""))[0]:
        WORST[tag] = (worst, what)
    if worst > 1.0:
        g = got.detach().cpu().double()[idx]
        raise AssertionError(f"{what}: worst |got - ref| / bound = {worst:.4g} at {idx}: got {float(g)!r}, "
                             f"ref {float(ref[idx])!r}, bound {float(bound[idx])!r}")
    return worst


OUTPUTS = ("O", "lse", "dQ", "dK", "dV", "dbias")


def ratios(got, R, bd):
    """{output: worst ratio} of a result dict in reference layout (missing outputs skipped)."""
    return {n: ratio(got[n], getattr(R, n), bd[n])[0] for n in OUTPUTS if got.get(n) is not None and n in bd}


# ----------------------------------------------------------------------------
# fp32 CPU emulation of the kernels' arithmetic, and its mutants
# ----------------------------------------------------------------------------
def _rnd(x, T):
    return x.to(T).float()


def _f32c(x):
    return float(torch.tensor(x, dtype=torch.float32))


# name -> the class of (case, dtype) the mutant must be rejected on
MUTANTS = {
    "drop_last_ragged_key": lambda c, T: c.Sk % 64 != 0 and c.Sk > 1,
    "causal_plus1": lambda c, T: c.causal,
    "causal_minus1": lambda c, T: c.causal,
    "skip_block32": lambda c, T: c.Sq >= 32 and c.Sk >= 32,
    "swap_v_rows": lambda c, T: c.Sk >= 2,
    "klens_wrong_batch": lambda c, T: c.k_lens is not None and len(set(c.k_lens)) > 1,
    "kv_head_mod": lambda c, T: 1 < c.Hk < c.H,
    "delta_scaled": lambda c, T: True,
    "dq_scaled": lambda c, T: True,
    "lse_shift": lambda c, T: True,
    "drop_rescale_1mp": lambda c, T: c.p > 0 and c.p != 0.5,
    "drop_other_half": lambda c, T: c.p > 0 and c.Sk > 4,
    "bias_before_scale": lambda c, T: c.bias != "none",
    "dbias_unreduced": lambda c, T: c.trainable and c.bias in ("key", "bq"),
    # the two below move a rounding to 16 bits: they do not exist in the fp32 unit
    "ds_from_rounded_p": lambda c, T: T != F32,
    "delta_unrounded_o": lambda c, T: T != F32,
}
MUTANTS_16BIT_ONLY = ("ds_from_rounded_p", "delta_unrounded_o")
# ("P not rounded to T before the PV product" is not in the list: it only removes a rounding, so its result is
# closer to the float64 reference than the kernel's and no error bound can reject it; emulate() still has it,
# as mut="p_unrounded", and tests/test_attn_reference.py asserts that it stays inside the bound.)
# "dS rounded twice" is here as ds_from_rounded_p (dS formed from the P already rounded to T, then rounded
# again): rounding dS itself to T a second time is idempotent and changes nothing.
# Strength of the three relative perturbations (delta, dQ, lse): 8 u in every dtype. In the fp32 unit that is
# 8 * 2**-24, which only the "sharp" cases reject (one nonzero per row of q and dO, two or three keys: every
# dot product is a single product and the bound a handful of roundings).
MUT_EPS = {T: 8 * HALF_ULP[T] for T in (BF16, F16, F32)}


def emulate(ops, T, p_nominal=0.0, mut=None):
    """The kernels' arithmetic in fp32 with roundings to T at their points: online softmax per key tile
    with the alpha rescale, P rounded to T and the keep mask applied to the rounded P, the epilogue
    inv = drop_scale / l; backward: P recomputed from the stored lse, delta from the stored O (fused and
    pre-pass kernels alike), dS and P rounded to T for the dK / dQ / dV products. T = F32: the fp32 unit
    (32-key tiles, scale folded into Q, no rounding to 16 bits). Returns a dict in reference layout."""
    B, H, Hk, Sq, Sk, D = ops.dims
    f32 = T == F32
    rT = (lambda x: x) if f32 else (lambda x: _rnd(x, T))
    tile = FWD_TILE[T]
    scale = _f32c(ops.scale)
    q, do = bh(ops.q.float()), bh(ops.do.float())
    k, v = _kv_bh(ops.k, H, mut).float(), _kv_bh(ops.v, H, mut).float()
    vf = v
    if mut == "swap_v_rows":
        vf = v.clone()
        vf[:, :, [0, 1]] = v[:, :, [1, 0]]
    bias = None if ops.bias is None else ops.bias.float()
    vis = visible(ops, mut).expand(B, H, Sq, Sk)
    keep = None if ops.keep is None else ops.keep
    if keep is not None and mut == "drop_other_half":
        idx = torch.arange(Sk) ^ 4
        idx = torch.where(idx < Sk, idx, torch.arange(Sk))
        keep = keep[..., idx]
    keepf = torch.ones(B, H, Sq, Sk) if keep is None else keep.float()
    r = _f32c(1.0 / (1.0 - p_nominal) if (mut == "drop_rescale_1mp" and ops.thresh) else ops.r)
    natural = f32 or bias is not None               # scores taken to the natural domain before the exp2
    sl2 = _f32c(LOG2E) if natural else _f32c(ops.scale * LOG2E)
    qs = q * scale if f32 else q                    # the fp32 unit folds the scale into Q

    def scores(k0, k1):
        s = qs @ k[:, :, k0:k1].transpose(-1, -2)
        if bias is not None:
            bt = bias[..., k0:k1]
            if mut == "bias_before_scale":
                s = (s + bt) * scale if not f32 else s + bt * scale
            else:
                s = s + bt if f32 else s * scale + bt
        return s

    NEG = torch.tensor(-INF)
    m = torch.full((B, H, Sq, 1), -INF)
    l = torch.zeros(B, H, Sq, 1)
    o = torch.zeros(B, H, Sq, D)
    for k0 in range(0, Sk, tile):
        k1 = min(Sk, k0 + tile)
        s = torch.where(vis[..., k0:k1], scores(k0, k1), NEG)
        if mut == "skip_block32" and k0 == 0:
            s[:, :, :32, :32] = -INF
        mnew = torch.maximum(m, s.max(-1, keepdim=True).values)
        muse = torch.where(mnew == -INF, torch.zeros_like(mnew), mnew)
        alpha = torch.exp2((m - muse) * sl2)
        p = torch.exp2(s * sl2 + (-muse * sl2))
        m = mnew
        l = l * alpha + p.sum(-1, keepdim=True)
        pr = p if mut == "p_unrounded" else rT(p)
        o = o * alpha + (pr * keepf[..., k0:k1]) @ vf[:, :, k0:k1]
    live = l > 0
    inv = torch.where(live, r / l.clamp(min=1e-37), torch.zeros_like(l))
    o_acc = o * inv
    O = rT(o_acc)
    ms = torch.where(live, m, torch.zeros_like(m))
    lse = (ms + torch.log(l.clamp(min=1e-37))) if f32 else (ms * sl2 + torch.log2(l.clamp(min=1e-37))) * _f32c(LN2)
    lse = torch.where(live, lse, torch.full_like(lse, INF))
    if mut == "lse_shift":
        lse = lse * (1 + MUT_EPS[T]) + MUT_EPS[T]
    # backward
    s = qs @ k.transpose(-1, -2)
    if f32:
        x = ((s if bias is None else s + bias) - lse) * sl2
    else:
        lse2 = lse * _f32c(LOG2E)
        sl2b = _f32c(ops.scale * LOG2E)
        if bias is not None and mut == "bias_before_scale":
            x = (s + bias) * sl2b - lse2
        else:
            x = s * sl2b + (-lse2 if bias is None else bias * _f32c(LOG2E) - lse2)
    p = torch.where(vis & (lse < INF), torch.exp2(x), torch.zeros_like(x))
    dp = do @ v.transpose(-1, -2)
    od = o_acc if mut == "delta_unrounded_o" else O
    delta = (od * do).sum(-1, keepdim=True)
    if mut == "delta_scaled":
        delta = delta * (1 - MUT_EPS[T])
    pds = rT(p) if mut == "ds_from_rounded_p" else p
    ds = pds * (dp * keepf * r - delta)
    dsr = rT(ds)
    dVx = rT((rT(p * keepf).transpose(-1, -2) @ do) * r)
    dKx = rT(dsr.transpose(-1, -2) @ qs) if f32 else rT((dsr.transpose(-1, -2) @ q) * scale)
    dQ = rT((dsr @ k) * scale)
    if mut == "dq_scaled":
        dQ = rT(dQ * (1 + MUT_EPS[T]))
    g = H // Hk
    if g == 1:
        dK, dV = dKx, dVx
    else:
        dK, dV = rT(dKx.view(B, Hk, g, Sk, D).sum(2)), rT(dVx.view(B, Hk, g, Sk, D).sum(2))
    dbias = None
    if bias is not None:
        dbias = reduce_to(ds, bias.shape)
        if mut == "dbias_unreduced":
            first = ds
            for i in range(3):
                if bias.shape[i] == 1:
                    first = first.narrow(i, 0, 1)
            dbias = first
    return {"O": O, "lse": lse.squeeze(-1), "dQ": dQ, "dK": dK, "dV": dV, "dbias": dbias}


def emu_stored(E):
    """(o_stored [B, Sq, H, D], lse_stored) of an emulation result, for reference()."""
    return E["O"].permute(0, 2, 1, 3), E["lse"]


# ----------------------------------------------------------------------------
# cases and seeded generators
# ----------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    Sq: int
    Sk: int
    D: int = 64
    B: int = 2
    H: int = 3
    Hk: int = 0            # 0: H
    causal: bool = False
    p: float = 0.0
    bias: str = "none"     # "key" [1, H, 1, Sk] | "bq" [B, 1, Sq, Sk] | "full" [B, H, Sq, Sk]
    bias_inf: bool = False
    trainable: bool = False
    k_lens: tuple | None = None
    kind: str = "normal"   # "big" | "corr" | "pos" | "sharp" | "sharpd" | "sharpbig"
    layout: str = "plain"  # "packed" | "gpacked" | "strided" | "padded"
    dsum: bool = False
    dtypes: tuple = (BF16, F16, F32)

    def __post_init__(self):
        if not self.Hk:
            object.__setattr__(self, "Hk", self.H)
        if self.D > 128:
            object.__setattr__(self, "dtypes", tuple(t for t in self.dtypes if t != F32))

    @property
    def scale(self):
        return 1.0 / math.sqrt(self.D)

    @property
    def thresh(self):
        return drop_thresh(self.p)

    @property
    def seed_offset(self):
        c = zlib.crc32(self.name.encode())
        return 0x1234_5678_0000 + c, 0x7777_0000_0000 + (c >> 3)


SK_SHORT, SK_LONG = (1, 33, 64, 65, 128), (129, 192, 193, 257, 320)
SQS = (1, 33, 128, 129, 160)
BIAS_FORMS = ("key", "bq", "full")


def sweep_cases():
    """One case per head dim x key class x causal x dropout x bias: the key lengths walk through the tile and
    kernel-choice boundaries, the query counts through SQS independently of them; self-attention (packed
    layout, with the bias-gradient column sums) where there is neither a bias nor a causal cross shape."""
    out = []
    i = 0
    for D in (32, 64, 128, 256):
        for long in (False, True):
            for causal in (False, True):
                for drop in (False, True):
                    for bias in (False, True):
                        Sk = (SK_LONG if long else SK_SHORT)[(i + i // 5) % 5]
                        dsum = not bias and D in (32, 128)
                        Sq = Sk if dsum or (causal and i % 2) else SQS[(i // 2 + i // 7) % 5]
                        BH = ((2, 3), (1, 2), (2, 1))[i % 3]
                        kl = None
                        if i % 4 == 1 and Sk > 1:
                            kl = (Sk, max(1, Sk // 2))[:BH[0]]
                        form = BIAS_FORMS[(i // 2) % 3] if bias else "none"
                        out.append(Case(
                            f"sw-d{D}-{'l' if long else 's'}{Sk}x{Sq}{'-c' if causal else ''}{'-p' if drop else ''}"
                            f"{'-b' + form if bias else ''}", Sq, Sk, D, BH[0], BH[1], causal=causal,
                            p=(0.1, 0.5)[(i // 3) % 2] if drop else 0.0, bias=form, bias_inf=bias and i % 4 == 3,
                            trainable=bias and (i // 4) % 2 == 0, k_lens=kl, layout="packed" if dsum else "plain",
                            dsum=dsum))
                        i += 1
    return out


SPECIAL = [
    # the fused backward over several query blocks; the two-kernel scheme with few queries
    Case("x160-96", 160, 96, p=0.5, k_lens=(96, 1)),
    Case("x40-200", 40, 200, D=32, bias="bq", trainable=True, k_lens=(0, 200)),
    # causal self-attention over three query blocks, qstart > 0 in the second and third key blocks
    Case("c257", 257, 257, causal=True, p=0.1, k_lens=(257, 130)),
    Case("c320", 320, 320, D=128, causal=True, bias="full", bias_inf=True, trainable=True),
    Case("c257-key", 257, 257, D=32, causal=True, bias="key", bias_inf=True, trainable=True, p=0.5, k_lens=(200, 257)),
    # grouped-query attention (group 2: H = 4 is the one case above three heads, so that h // group and
    # h % Hk differ) and multi-query, ragged lengths; the grouped packed layout
    Case("gqa-g2", 77, 77, B=1, H=4, Hk=2, causal=True),
    Case("mqa", 33, 150, H=3, Hk=1, p=0.1),
    Case("gpacked", 200, 200, H=2, Hk=1, p=0.1, layout="gpacked"),
    Case("gpacked-s", 77, 77, H=2, Hk=1, causal=True, layout="gpacked"),
    # scores up to ~50 (max subtraction, the lse round trip); dO correlated with O (a large delta)
    Case("big", 96, 257, kind="big"),
    Case("big-c", 129, 129, D=128, causal=True, kind="big"),
    Case("corr", 160, 160, kind="corr"),
    Case("corr-l", 33, 193, D=32, kind="corr", p=0.1),
    # a high dropout rate over non-negative V: 256 / (256 - thresh) and 1 / (1 - p) are 1.5 % apart
    Case("drophi", 64, 96, kind="pos", p=0.9),
    # sparse q and dO: scores, dP and delta are single products, the bound is a few roundings
    Case("sharp", 5, 3, D=32, B=1, H=2, kind="sharp"),
    Case("sharp-b", 33, 2, D=32, B=2, H=1, kind="sharp", bias="key", trainable=True),
    # the same with V = 1 + small: dP and delta nearly cancel in dS, so an error of delta is amplified
    Case("sharp-d", 5, 3, D=32, B=1, H=2, kind="sharpd"),
    # many rows of the same: the worst element of a few thousand is what the floor of the CPU test looks at; a
    # stored (not added) bias gradient; and scores of +-50 with exact products (|lse| ~ 50 against a bound of
    # a few roundings of it)
    Case("sharp-l", 320, 2, D=32, kind="sharp"),
    Case("sharp-f", 320, 3, D=32, kind="sharp", bias="full", trainable=True),
    Case("sharp-big", 128, 3, D=32, kind="sharpbig"),
    # column sums over gradients of very different magnitudes (sums of like-sized 16-bit values are exact in fp32)
    Case("big-ds", 128, 128, D=32, kind="big", layout="packed", dsum=True),
    Case("big-dl", 257, 257, causal=True, kind="big", layout="packed", dsum=True),
    Case("big-d3", 3, 3, D=128, kind="big", layout="packed", dsum=True),
    Case("big-d9", 9, 9, D=256, kind="big", layout="packed", dsum=True),
    Case("strided", 129, 192, bias="key", p=0.5, layout="strided"),
    Case("padded80", 65, 129, D=80, causal=False, layout="padded"),
]


def all_cases():
    return sweep_cases() + SPECIAL


def operands(case, T):
    """Seeded operands of a case in T on the CPU, as an Ops (keep from keep_mask with the case's seed)."""
    c = case
    g = _gen(f"{c.name}-{DT_NAME[T]}")
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    q, k, v = rn(c.B, c.Sq, c.H, c.D), rn(c.B, c.Sk, c.Hk, c.D), rn(c.B, c.Sk, c.Hk, c.D)
    do = rn(c.B, c.Sq, c.H, c.D)
    if c.kind == "big":
        q = q * 10.5           # |q.k| * scale reaches 44 - 51
    if c.kind == "pos":
        v = v.abs()
    if c.kind == "sharpd":
        v = 1.0 + 0.02 * v
    if c.kind in ("sharp", "sharpd", "sharpbig"):      # one nonzero per row of q and dO
        for t in (q, do):
            idx = torch.randint(0, c.D, t.shape[:-1] + (1,), generator=g)
            t.mul_(torch.zeros_like(t).scatter_(-1, idx, 1.0))
        q = q * (90.0 if c.kind == "sharpbig" else 3.0)
    bias = None
    if c.bias != "none":
        shape = {"key": (1, c.H, 1, c.Sk), "bq": (c.B, 1, c.Sq, c.Sk), "full": (c.B, c.H, c.Sq, c.Sk)}[c.bias]
        bias = rn(*shape)
        if c.bias_inf:
            bias = bias.masked_fill(torch.rand(shape, generator=g) < 0.1, -INF)
            if c.bias == "full":
                bias[0, 0, min(1, c.Sq - 1)] = -INF    # one fully masked row
        bias = bias.to(T)
    q, k, v, do = (t.to(T) for t in (q, k, v, do))
    keep = None
    if c.p > 0:
        seed, off = c.seed_offset
        keep = torch.from_numpy(keep_mask(seed, off, c.B * c.H, c.Sq, c.Sk, c.thresh)).view(c.B, c.H, c.Sq, c.Sk)
    ops = Ops(q, k, v, do, c.scale, c.causal, c.k_lens, bias, keep, c.thresh)
    if c.kind == "corr":
        o = reference(ops).O.permute(0, 2, 1, 3)
        ops = replace(ops, do=(4.0 * o + 0.05 * do.double()).to(T))
    return ops


# ----------------------------------------------------------------------------
# exact cases
# ----------------------------------------------------------------------------
def onehot_perm(Sq, Sk, causal):
    """pi(q): the one key query q sees. Causal: pi(q) = q (the only map with pi(q) <= q that hits every key of a
    square shape); otherwise an affine map mod Sk (a permutation when Sq == Sk: 7 is coprime to every Sk used)."""
    qi = torch.arange(Sq)
    return torch.minimum(qi, torch.tensor(Sk - 1)) if causal else (7 * qi + 3) % Sk


def onehot_operands(B, H, Sq, Sk, D, T, causal):
    """q = 0 and a 0 / -inf bias that leaves key pi(q) alone: O[q] = V[pi(q)] bit for bit, lse = 0,
    dV[k] = the sum of dO[q] over pi(q) = k (small integers: exact in any order), dK = dQ = 0 (dP = delta
    exactly: sums of the same integer products)."""
    g = _gen(f"onehot-{B}-{H}-{Sq}-{Sk}-{D}")
    pi = onehot_perm(Sq, Sk, causal)
    bias = torch.full((B, H, Sq, Sk), -INF)
    bias[:, :, torch.arange(Sq), pi] = 0.0
    v = torch.randint(-8, 9, (B, Sk, H, D), generator=g).float()
    v[..., 0] = torch.arange(Sk).float()[None, :, None] % 251          # no two keys alike
    v[..., 1] = (torch.arange(Sk) // 251).float()[None, :, None] + torch.arange(H).float()[None, None, :]
    do = torch.randint(-4, 5, (B, Sq, H, D), generator=g).float()
    k = torch.randn(B, Sk, H, D, generator=g)
    ops = Ops(torch.zeros(B, Sq, H, D).to(T), k.to(T), v.to(T), do.to(T), 1.0 / math.sqrt(D), causal, None, bias.to(T))
    dv = torch.zeros(B, Sk, H, D).index_add_(1, pi, do)
    return ops, {"O": v[:, pi], "dV": dv, "pi": pi}


def uniform_operands(B, H, Sq, Sk, n, D, T, keep=None):
    """q = 0, no bias, n visible keys (Sk itself, or k_lens = n inside a ragged Sk): P = 1 / n on every visible
    key. V[k, d] = bit (d mod 9) of k + 1 and small-integer dO: n O (n O / 2 with the p = 0.5 keep mask, whose
    rescale is exactly 2) is the count of (kept) keys per bit and n dV the (kept) column sum of dO — integers,
    exact in T for n a power of two up to 256."""
    g = _gen(f"uniform-{B}-{H}-{Sq}-{Sk}-{n}-{D}")
    kk = torch.arange(Sk)[:, None] + 1
    v = ((kk >> (torch.arange(D)[None, :] % 9)) & 1).float()[None, :, None, :].expand(B, Sk, H, D).contiguous()
    do = torch.randint(-2, 3, (B, Sq, H, D), generator=g).float()
    k = torch.randn(B, Sk, H, D, generator=g)
    r = 1.0 if keep is None else 2.0
    ops = Ops(torch.zeros(B, Sq, H, D).to(T), k.to(T), v.to(T), do.to(T), 1.0 / math.sqrt(D), False,
              None if n == Sk else (n,) * B, None, keep, 0 if keep is None else 128)
    kf = torch.ones(B, H, Sq, Sk) if keep is None else keep.float()
    kf = kf * (torch.arange(Sk) < n).float()
    O = torch.einsum("bhqk,bkhd->bqhd", kf, v) * (r / n)
    dV = torch.einsum("bhqk,bqhd->bkhd", kf, do) * (r / n)
    return ops, {"O": O, "dV": dV, "lse": math.log(n)}


# (Sq, Sk, n visible keys, D): the short single-stage forward (D = 64, Sk <= 128), the two-barrier and the
# double-buffered loops, the fused and the two-kernel backward, n from Sk itself and from k_lens
UNIFORM_SHAPES = [(33, 64, 64, 64), (129, 128, 128, 64), (40, 100, 64, 64), (65, 256, 256, 64), (33, 300, 256, 128),
                  (129, 129, 128, 32), (33, 200, 128, 256)]
ONEHOT_SHAPES = [(65, 65, 64, False), (128, 128, 64, True), (193, 193, 64, False), (257, 257, 128, True),
                 (40, 200, 32, False), (160, 96, 256, False), (129, 320, 32, False)]
