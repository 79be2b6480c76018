"""MXFP4 on the device (csrc/mx.hip format 2, csrc/gemm_mx4.hip) against tests/mx4_reference.py, for both products
(e2m1 x e2m1 and fp8 x e2m1). Figures are printed before they are asserted."""
import functools

import pytest
import torch

import fp8_reference as F
import gemm_reference as R
import mx4_reference as X4
import mx_reference as X

pytestmark = pytest.mark.gpu
DEV, F32, BF16, E4M3, E5M2, E2M1 = "cuda", F.F32, F.BF16, F.E4M3, F.E5M2, X4.E2M1
K0 = {E2M1: 256, E4M3: 128, E5M2: 128}      # smallest K by the format of a (mx_supported's docstring)
PRODUCTS = pytest.mark.parametrize("fa", [E2M1, E4M3, E5M2], ids=["e2m1", "e4m3", "e5m2"])


def _fp8():
    import apex.fp8

    return apex.fp8


def _gemm(a, sa, b, sb, fa, bias, odt):
    return _fp8().mx_gemm(a.to(DEV), sa.to(DEV), b.to(DEV), sb.to(DEV), fa, E2M1, None if bias is None else bias.to(DEV), odt)


def _a_values(a, sa, fa):
    return X4.scaled(a, sa) if fa == E2M1 else X.scaled(a, sa, fa)


@PRODUCTS
@pytest.mark.parametrize("M,N,kt", [(16, 16, 1), (256, 256, 1), (256, 256, 3), (1, 8, 1), (300, 392, 2)])
def test_placement(M, N, kt, fa):
    """Integers with a different power-of-two scale on every 32-block of a K-tile: every partial sum is a multiple
    of 2**-6 below 2**24, so fp32 must equal float64 — a wrong lane, nibble, block, byte or stage changes it."""
    K, nb = kt * K0[fa], K0[fa] // 32
    assert _fp8().mx_supported(M, K, N, True, fa, E2M1) and not _fp8().mx_supported(M, K0[fa] // 2, N, True, fa, E2M1)
    g = R._gen(f"mx4-place-{M}-{N}-{K}-{fa}")
    ints = torch.tensor([0, 2, 4, 5, 10, 12, 13])            # e2m1 codes of 0, +-1, +-2, +-3
    B4 = X4.pack(ints[torch.randint(0, 7, (N, K), generator=g)])
    A = X4.pack(ints[torch.randint(0, 7, (M, K), generator=g)]) if fa == E2M1 else \
        F.encode(torch.randint(-4, 5, (M, K), generator=g), fa)
    sa, sb = ((torch.rand(r, kt, 8, generator=g).argsort(-1)[..., :nb] + 124).reshape(r, K // 32).to(torch.uint8)
              for r in (M, N))
    a, b = _a_values(A, sa, fa), X4.scaled(B4, sb)
    assert float((a.abs() @ b.abs().t()).max()) * 64 < 2 ** 24
    bad = int((_gemm(A, sa, B4, sb, fa, None, F32).cpu().double() != a @ b.t()).sum())
    print(f"placement {M}x{N}x{K} fa={fa}: {bad} of {M * N} differ")
    assert bad == 0


@functools.lru_cache(maxsize=None)
def _dense(M, N, K, fa):
    g = R._gen(f"mx4-dense-{M}-{N}-{K}-{fa}")
    B4 = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8)
    A = torch.randint(0, 256, (M, K // 2), generator=g).to(torch.uint8) if fa == E2M1 else F.dense_codes(f"mx4-a-{M}-{K}", M, K, fa)
    sa, sb = (torch.randint(119, 136, (r, K // 32), generator=g).to(torch.uint8) for r in (M, N))
    return A, sa, B4, sb, torch.randn(N, generator=g), _a_values(A, sa, fa), X4.scaled(B4, sb)


@pytest.mark.parametrize("with_bias", [False, True], ids=["none", "bias"])
@pytest.mark.parametrize("odt", [F32, BF16], ids=["fp32", "bf16"])
@PRODUCTS
@pytest.mark.parametrize("M,N,kt", [(256, 256, 1), (257, 264, 2), (300, 392, 3)])
def test_dense(M, N, kt, fa, odt, with_bias):
    """Full-range nibbles, scale bytes in 119 .. 135, within mx_reference's bound (worst accumulator figure measured
    on an MI355X: 669 units of 2**-24 cond, fp8 x fp4 at K = 256, under ACC_MX's 1024; fp4 x fp4 stays below 4)."""
    K = kt * K0[fa]
    A, sa, B4, sb, bias, a, b = _dense(M, N, K, fa)
    bias = bias.to(odt) if with_bias else None
    got = _gemm(A, sa, B4, sb, fa, bias, odt)
    assert got.dtype == odt and got.shape == (M, N)
    ref, bound = X4.expected(a, b, K, odt, bias)
    err = (got.cpu().double() - ref).abs()
    print(f"dense {M}x{N}x{K} fa={fa} {odt} bias={with_bias}: |err| / (2**-24 cond) "
          f"{float((err / (X.E24 * (a.abs() @ b.abs().t()))).max()):.4g}, |err| / bound {float((err / bound).max()):.4g}")
    assert bool((err <= bound).all())


def _quant_input(R_, C, dt):
    """randn scaled per 32-block by 2**uniform(-20, 20); the first blocks (as many as there are) replaced by: all zero,
    fp32 subnormals, an amax in the saturating interval (6, 8) 2**5, every tie (times 2**3), one NaN, one -inf."""
    g = R._gen(f"mx4-q-{R_}-{C}")
    x = torch.randn(R_, C // 32, 32, generator=g) * torch.exp2(torch.rand(R_, C // 32, 1, generator=g) * 40 - 20)
    sat_blk, nan_blk, inf_blk = (torch.randn(32, generator=g) for _ in range(3))
    sat_blk[7], nan_blk[3], inf_blk[30] = -7.0 * 32, float("nan"), float("-inf")
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0])
    special = [torch.zeros(32), torch.randn(32, generator=g) * 2.0 ** -140, sat_blk, torch.cat([ties, -ties] * 2) * 8, nan_blk, inf_blk]
    xb = x.reshape(-1, 32)
    for i, s in enumerate(special[:xb.shape[0]]):
        xb[i * (xb.shape[0] // len(special) or 1) % xb.shape[0]] = s
    return x.reshape(R_, C).to(dt)


@pytest.mark.parametrize("dt", [BF16, F.F16, F32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("R_,C", [(32, 32), (64, 96), (160, 224), (1, 64)])
def test_quantize(R_, C, dt):
    x, col = _quant_input(R_, C, dt), R_ % 32 == 0
    want = X4.quantize_ref(x) + (X4.quantize_ref(x.t()) if col else ())
    got = _fp8().mx_quantize(x.to(DEV), E2M1, True, col)
    for name, g_, w in zip(("row codes", "row scales", "col codes", "col scales"), got[0] + got[1] if col else got, want):
        bad = int((g_.cpu() != w).sum()) if g_.shape == w.shape else -1
        print(f"quantize {R_}x{C} {name}: {bad} of {w.numel()} differ")
        assert bad == 0


@PRODUCTS
def test_nan_scale(fa):
    """An fp4 row with a 0xFF block: that row (column) of the output is NaN, whatever the block's codes, and nothing
    else is — what gemm_mx.hip records for fp8."""
    K = K0[fa]
    A = torch.full((16, K // 2), 0x22, dtype=torch.uint8) if fa == E2M1 else F.encode(torch.ones(16, K), fa)
    B4 = torch.full((16, K // 2), 0x22, dtype=torch.uint8)
    sa, sb = (torch.full((16, K // 32), 127, dtype=torch.uint8) for _ in range(2))
    sb[9, 0], sb[5, K // 32 - 1], B4[5, -16:] = 0xFF, 0xFF, 0      # column 5: a marked block whose codes are all zero
    want = torch.full((16, 16), float(K))
    want[:, 9], want[:, 5] = float("nan"), float("nan")
    if fa == E2M1:
        sa[3, 2], want[3] = 0xFF, float("nan")
    got = _gemm(A, sa, B4, sb, fa, None, F32).cpu()
    print("0xFF scale: row 3", got[3, :4].tolist(), "row 0", got[0, 3:11].tolist())
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(), want.nan_to_num())


@pytest.mark.parametrize("N,main_grad", [(384, False), (384, True), (8, False)], ids=["n384", "main_grad", "dgrad_declined"])
@pytest.mark.parametrize("fwd,wfmt", [("e4m3", "e2m1"), ("e2m1", None)], ids=["w4", "x4w4"])
def test_linear(fwd, wfmt, N, main_grad):
    fp8, f = _fp8(), (E2M1 if fwd == "e2m1" else E4M3)
    sup = fp8.mx_supported
    M = K = next(k for k in (128, 256) if sup(k, k, 384, True, f, E2M1) and sup(k, 384, k, True, E5M2, E2M1) and sup(384, k, k, True, E5M2, f))
    assert sup(M, K, N, True, f, E2M1) and sup(M, N, K, True, E5M2, E2M1) == (N == 384)
    g = R._gen(f"mx4-linear-{M}-{N}")
    x, w, bias, dy = (torch.randn(*s, generator=g).to(BF16) for s in ((M, K), (N, K), (N,), (M, N)))
    exp = X4.linear_expected(x, w, bias, dy, f, E5M2, E2M1, sup)
    xd, wd, bd = (t.to(DEV).requires_grad_() for t in (x, w, bias))
    if main_grad:
        wd.main_grad = torch.full((N, K), 0.5, device=DEV)
    y = fp8.mx_linear(xd, wd, bd, fwd_format=fwd, weight_format=wfmt)
    y.backward(dy.to(DEV))
    ref, bound = exp["dw"]
    if main_grad:
        dw, ref = wd.main_grad, ref + 0.5
        bound = bound + X.HALF_ULP[F32] * ref.abs()
    else:
        dw, bound = wd.grad, bound + X.HALF_ULP[BF16] * ref.abs() + X.TINY[BF16]
    for name, got, (r_, b_) in (("y", y, exp["y"]), ("dx", xd.grad, exp["dx"]), ("db", bd.grad, exp["db"]), ("dw", dw, (ref, bound))):
        ratio = float(((got.detach().cpu().double() - r_).abs() / b_).max())
        print(f"linear {fwd}/{wfmt} {M}x{K}x{N} {name}: worst |err| / bound {ratio:.4g}")
        assert ratio <= 1.0, name
