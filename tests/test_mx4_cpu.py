"""MXFP4 on CPU tensors (the torch path of apex/fp8/mx.py) against tests/mx4_reference.py, and the refusals."""
import functools

import pytest
import torch

import fp8_reference as F
import gemm_reference as R
import mx4_reference as X4

E2M1 = X4.E2M1


def test_quantize_gemm_cpu():
    import apex.fp8 as fp8

    assert fp8.E2M1 == E2M1 and "e2m1" not in fp8._FMT_NAMES
    g = R._gen("mx4-cpu")
    x, w = torch.randn(64, 128, generator=g), torch.randn(16, 128, generator=g)
    x[0, :16] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0] * 2) * 4     # ties, a saturating amax
    x[1, 40], x[2, 70] = float("nan"), float("-inf")
    row, col = fp8.mx_quantize(x, "e2m1", True, True)
    for got, want in zip(row + col, X4.quantize_ref(x) + X4.quantize_ref(x.t())):
        assert got.shape == want.shape and torch.equal(got, want)
    w4 = fp8.mx_quantize(w, E2M1)
    assert torch.equal(fp8.mx_dequantize(*w4, E2M1, torch.float64), X4.scaled(*w4))
    x = x.nan_to_num(0.0, 0.0, 0.0)
    for fa in (E2M1, F.E4M3):
        ref, bound = X4.expected(X4.operand(x, fa), X4.scaled(*w4), 128, torch.float32)
        got = fp8.mx_gemm(*fp8.mx_quantize(x, fa), *w4, fa, E2M1, None, torch.float32)
        assert bool(((got.double() - ref).abs() <= bound).all())
    x8 = fp8.mx_quantize(x, F.E4M3)
    for bad in (lambda: fp8.mx_gemm(*w4, *x8, E2M1, F.E4M3),                           # a fp4 with b fp8
                lambda: fp8.mx_gemm(*x8, w4[0].repeat(1, 2), w4[1], F.E4M3, E2M1),     # b not packed [N, K / 2]
                lambda: fp8.mx_linear(x, w, None, bwd_format="e2m1")):
        with pytest.raises(ValueError):
            bad()
    assert not fp8.mx_supported(64, 128, 16, False, E2M1, F.E4M3)


@pytest.mark.parametrize("fwd,wfmt", [("e4m3", "e2m1"), ("e2m1", None)], ids=["w4", "x4w4"])
def test_linear_cpu(fwd, wfmt):
    import apex.fp8 as fp8

    g = R._gen("mx4-linear-cpu")
    x, w, bias, dy = (torch.randn(*s, generator=g) for s in ((64, 128), (16, 128), (16,), (64, 16)))
    exp = X4.linear_expected(x, w, bias, dy, E2M1 if fwd == "e2m1" else F.E4M3, F.E5M2, E2M1,
                             functools.partial(fp8.mx_supported, native=False))
    xg, wg, bg = (t.clone().requires_grad_() for t in (x, w, bias))
    y = fp8.mx_linear(xg, wg, bg, fwd_format=fwd, weight_format=wfmt)
    y.backward(dy)
    for name, got in (("y", y), ("dx", xg.grad), ("dw", wg.grad), ("db", bg.grad)):
        ratio = float(((got.detach().double() - exp[name][0]).abs() / exp[name][1]).max())
        print(f"cpu linear {fwd}/{wfmt} {name}: worst |err| / bound {ratio:.4g}")
        assert ratio <= 1.0, name
