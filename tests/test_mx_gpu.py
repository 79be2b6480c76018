"""MXFP8 on the device (csrc/mx.hip, csrc/gemm_mx.hip, apex/fp8/mx.py) against tests/mx_reference.py: the lane /
block / scale mapping of the scaled MFMA with integers, dense products against float64, the quantiser to the bit,
the measured 0xFF-scale behaviour, and mx_linear's three GEMMs. Every test prints its figures before asserting;
MX_NUMERICS_WORST_OUT names a file that receives the worst accumulator error of the dense cases."""
import functools
import os

import pytest
import torch

import fp8_reference as F
import gemm_reference as R
import mx_reference as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F16, BF16 = F.F32, F.F16, F.BF16
E4M3, E5M2 = F.E4M3, F.E5M2
FMT_IDS = lambda f: F.FMT_NAME[f]  # noqa: E731
DT_IDS = lambda t: F.DT_NAME[t]  # noqa: E731
WORST = {"acc": 0.0}


def _fp8():
    import apex.fp8

    return apex.fp8


@pytest.fixture(scope="module", autouse=True)
def _worst_file():
    yield
    out = os.environ.get("MX_NUMERICS_WORST_OUT")
    if out:
        with open(out, "w") as f:
            f.write(f"worst |err| / (2**-24 cond), dense fp32 outputs without bias: {WORST['acc']:.4g}\n")


def _within(got, ref, bound, what):
    err = (got.detach().cpu().double() - ref).abs()
    ratio = float((err / bound).max())
    print(f"{what}: worst |err| / bound {ratio:.4g}")
    assert ratio <= 1.0, f"{what}: |err| / bound {ratio:.4g}"
    return ratio


# ---- 1. scale placement, exact ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fa", [E4M3, E5M2], ids=FMT_IDS)
@pytest.mark.parametrize("M,N,K", [(16, 16, 128), (256, 256, 128), (256, 256, 384), (1, 8, 128), (300, 392, 256)])
def test_scale_placement(M, N, K, fa):
    """Small integers with a different power-of-two scale on each of a K-tile's four blocks: every partial sum is
    a multiple of 2**-6 below 2**24, so fp32 must equal float64 — a wrong lane / block / byte / stage changes it."""
    g = R._gen(f"mx-place-{M}-{N}-{K}")
    A = torch.randint(-2, 3, (M, K), generator=g)
    B = torch.randint(-8, 9, (N, K), generator=g)
    sa, sb = ((torch.rand(r, K // 128, 7, generator=g).argsort(-1)[..., :4] + 124).reshape(r, K // 32).to(torch.uint8)
              for r in (M, N))
    A8, B8 = F.encode(A, fa), F.encode(B, E4M3)
    a, b = X.scaled(A8, sa, fa), X.scaled(B8, sb, E4M3)
    assert float((a.abs() @ b.abs().t()).max()) * 64 < 2 ** 24
    got = _fp8().mx_gemm(A8.to(DEV), sa.to(DEV), B8.to(DEV), sb.to(DEV), fa, E4M3, None, F32)
    bad = int((got.cpu().double() != a @ b.t()).sum())
    print(f"placement {M}x{N}x{K} {F.FMT_NAME[fa]}: {bad} of {M * N} differ")
    assert bad == 0


# ---- 2. dense GEMM against float64 ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense(M, N, K, fa):
    g = R._gen(f"mx-dense-{M}-{N}-{K}")
    A8, B8 = F.dense_codes(f"mx-a-{M}-{K}", M, K, fa), F.dense_codes(f"mx-b-{N}-{K}", N, K, E4M3)
    sa, sb = (torch.randint(119, 136, (r, K // 32), generator=g).to(torch.uint8) for r in (M, N))
    bias = torch.randn(N, generator=g)
    return A8, sa, B8, sb, bias, X.scaled(A8, sa, fa), X.scaled(B8, sb, E4M3)


@pytest.mark.parametrize("with_bias", [False, True], ids=["none", "bias"])
@pytest.mark.parametrize("odt", [F32, BF16], ids=DT_IDS)
@pytest.mark.parametrize("fa", [E4M3, E5M2], ids=FMT_IDS)
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (257, 264, 256), (300, 392, 384)])
def test_dense(M, N, K, fa, odt, with_bias):
    A8, sa, B8, sb, bias, a, b = _dense(M, N, K, fa)
    bias = bias.to(odt) if with_bias else None
    got = _fp8().mx_gemm(A8.to(DEV), sa.to(DEV), B8.to(DEV), sb.to(DEV), fa, E4M3,
                         None if bias is None else bias.to(DEV), odt)
    assert got.dtype == odt and got.shape == (M, N)
    ref, bound = X.expected(a, b, K, odt, bias)
    if odt == F32 and not with_bias:
        r = float(((got.cpu().double() - ref).abs() / (X.E24 * (a.abs() @ b.abs().t()))).max())
        WORST["acc"] = max(WORST["acc"], r)
        print(f"dense {M}x{N}x{K} {F.FMT_NAME[fa]}: |err| / (2**-24 cond) = {r:.4g}")
    _within(got, ref, bound, f"dense {M}x{N}x{K} {F.FMT_NAME[fa]} {F.DT_NAME[odt]} bias={with_bias}")


# ---- 3. quantiser to the bit ------------------------------------------------------------------------------------
def _quant_input(R_, C, dt, fmt):
    """randn scaled per 32-block by 2**uniform(-20, 20); the first blocks (as many as there are) replaced by: all
    zero, fp32 subnormals, an amax in the saturating interval, one NaN, one inf."""
    g = R._gen(f"mx-q-{R_}-{C}")
    x = torch.randn(R_, C // 32, 32, generator=g) * torch.exp2(torch.rand(R_, C // 32, 1, generator=g) * 40 - 20)
    top = (480.0 if fmt == E4M3 else 61440.0) * 2.0 ** (5 if fmt == E4M3 else -3)
    sat_blk, nan_blk, inf_blk = (torch.randn(32, generator=g) for _ in range(3))
    sat_blk[7], nan_blk[3], inf_blk[30] = -top, float("nan"), float("-inf")
    special = [torch.zeros(32), torch.randn(32, generator=g) * 2.0 ** -140, sat_blk, nan_blk, inf_blk]
    xb = x.reshape(-1, 32)
    for i, s in enumerate(special[:xb.shape[0]]):
        xb[i * (xb.shape[0] // len(special) or 1) % xb.shape[0]] = s
    return x.reshape(R_, C).to(dt)


def _same_pair(got, want, what):
    for name, g_, w in zip(("codes", "scales"), got, want):
        bad = int((g_.cpu() != w).sum())
        print(f"{what} {name}: {bad} of {w.numel()} differ")
        assert g_.shape == w.shape and bad == 0, f"{what} {name}: {bad} differ"


@pytest.mark.parametrize("fmt", [E4M3, E5M2], ids=FMT_IDS)
@pytest.mark.parametrize("dt", [BF16, F16, F32], ids=DT_IDS)
@pytest.mark.parametrize("R_,C", [(32, 32), (64, 96), (160, 224), (1, 64)])
def test_quantize(R_, C, dt, fmt):
    q = _fp8().mx_quantize
    x = _quant_input(R_, C, dt, fmt)
    row = q(x.to(DEV), fmt, True, False)
    _same_pair(row, X.quantize_ref(x, fmt), f"rowwise {R_}x{C}")
    if R_ % 32:
        return
    xt = _quant_input(C, R_, dt, fmt).t().contiguous()     # the special blocks along columns
    _same_pair(q(xt.to(DEV), fmt, False, True), X.quantize_ref(xt.t(), fmt), f"colwise {R_}x{C}")
    col = q(x.to(DEV), fmt, False, True)
    _same_pair(col, X.quantize_ref(x.t(), fmt), f"colwise of the rowwise input {R_}x{C}")
    both = q(x.to(DEV), fmt, True, True)
    for one, two in zip(row + col, both[0] + both[1]):
        assert torch.equal(one, two)


# ---- 4. a 0xFF scale through the GEMM ------------------------------------------------------------------------------
def test_nan_scale():
    """The measured behaviour stated in gemm_mx.hip's header and mx_gemm's docstring."""
    M = N = 16
    A8 = F.encode(torch.ones(M, 128), E4M3)
    B8 = F.encode(torch.ones(N, 128), E4M3)
    sa = torch.full((M, 4), 127, dtype=torch.uint8)
    sb = sa.clone()
    sa[3, 2] = 0xFF                      # row 3: a marked block with nonzero codes
    sa[5, 1] = 0xFF
    A8[5, 32:64] = 0                     # row 5: a marked block whose codes are all zero
    sb[9, 0] = 0xFF                      # column 9: a marked block of B
    got = _fp8().mx_gemm(A8.to(DEV), sa.to(DEV), B8.to(DEV), sb.to(DEV), E4M3, E4M3, None, F32).cpu()
    print("0xFF scale: row 3", got[3, :4].tolist(), "row 5", got[5, :4].tolist(), "row 0", got[0, 7:11].tolist())
    want = torch.full((M, N), 128.0)     # the hardware honours the E8M0 NaN: whole rows / columns, nothing else
    want[3], want[5], want[:, 9] = float("nan"), float("nan"), float("nan")
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(), want.nan_to_num())


# ---- 5. mx_linear ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N,main_grad", [(256, 256, 384, False), (384, 128, 8, False), (256, 256, 384, True)])
def test_linear(M, K, N, main_grad):
    fp8 = _fp8()
    g = R._gen(f"mx-linear-{M}-{K}-{N}")
    x, w, bias, dy = (torch.randn(*s, generator=g).to(BF16) for s in ((M, K), (N, K), (N,), (M, N)))
    exp = X.linear_expected(x, w, bias, dy, E4M3, E5M2, fp8.mx_supported)
    xd, wd, bd = (t.to(DEV).requires_grad_() for t in (x, w, bias))
    if main_grad:
        wd.main_grad = torch.full((N, K), 0.5, device=DEV)
    y = fp8.mx_linear(xd, wd, bd)
    y.backward(dy.to(DEV))
    ref, bound = exp["dw"]
    if main_grad:
        dw, ref = wd.main_grad, ref + 0.5
        bound = bound + X.HALF_ULP[F32] * ref.abs()
        assert dw.dtype == F32 and wd.grad_added_to_main_grad and (wd.grad is None or not bool(wd.grad.any()))
    else:
        dw, bound = wd.grad, bound + X.HALF_ULP[BF16] * ref.abs() + X.TINY[BF16]
    for name, got in (("y", y), ("dx", xd.grad), ("db", bd.grad)):
        _within(got, *exp[name], f"linear {M}x{K}x{N} {name}")
    _within(dw, ref, bound, f"linear {M}x{K}x{N} dw main_grad={main_grad}")


def test_linear_declined():
    """K = 100: not an MX shape, so the layer is torch.nn.functional.linear."""
    g = R._gen("mx-linear-declined")
    x, w, b = (torch.randn(*s, generator=g).to(BF16).to(DEV) for s in ((64, 100), (16, 100), (16,)))
    assert not _fp8().mx_supported(64, 100, 16)
    assert torch.equal(_fp8().mx_linear(x, w, b), torch.nn.functional.linear(x, w, b))
