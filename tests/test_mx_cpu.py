"""apex.fp8.mx_linear on CPU tensors (the torch reference path of apex/fp8/mx.py) against tests/mx_reference.py:
keeps the reference path's quantiser and the autograd wiring of the three GEMMs honest without a device."""
import functools

import torch

import fp8_reference as F
import gemm_reference as R
import mx_reference as X


def test_linear_cpu():
    import apex.fp8 as fp8

    M, K, N = 64, 64, 32
    g = R._gen("mx-linear-cpu")
    x, w, bias, dy = (torch.randn(*s, generator=g) for s in ((M, K), (N, K), (N,), (M, N)))
    for fmt in (F.E4M3, F.E5M2):     # the reference path's quantiser, to the bit, both orientations
        row, col = fp8.mx_quantize(x, fmt, True, True)
        for got, want in zip(row + col, X.quantize_ref(x, fmt) + X.quantize_ref(x.t(), fmt)):
            assert torch.equal(got, want)
    exp = X.linear_expected(x, w, bias, dy, F.E4M3, F.E5M2, functools.partial(fp8.mx_supported, native=False))
    xg, wg, bg = (t.clone().requires_grad_() for t in (x, w, bias))
    y = fp8.mx_linear(xg, wg, bg)
    y.backward(dy)
    for name, got in (("y", y), ("dx", xg.grad), ("dw", wg.grad), ("db", bg.grad)):
        ref, bound = exp[name]
        ratio = float(((got.detach().double() - ref).abs() / bound).max())
        print(f"cpu linear {name}: worst |err| / bound {ratio:.4g}")
        assert ratio <= 1.0, name
