"""The grouped MFMA GEMMs (csrc/gemm_grouped.hip) through apex.ops.grouped_linear, forward and backward, against
the float64 reference and the derived bounds of gemm_reference.py, expert by expert.

Segments: rows per expert [64, 0, 320, 256, 192] in R = 960 rows (a 128-row tail): an empty expert, a partial
tile, a 64-row start that is not tile-aligned, one exact tile, a tile plus a partial. "notail" appends an empty
last expert whose end is R = 832. K = 64 / 192: one K-tile and an odd count (both LDS buffers, the unroll-by-two
tail); N = 256 / 264: a full tile, and a full tile plus an 8-column edge."""
import functools
import math

import pytest
import torch

from gemm_reference import BF16, DT_NAME, DTYPES, F32, acc_ref, check, expected, wgrad_expected

pytestmark = pytest.mark.gpu

CASES = {"tail": ([64, 0, 320, 256, 192], 960), "notail": ([64, 0, 320, 256, 192, 0], 832)}
KS, NS = [64, 192], [256, 264]
ids = dict(ids=lambda v: DT_NAME.get(v, str(v)))


def _offsets(rows):
    return [sum(rows[:i]) for i in range(len(rows) + 1)]


@functools.lru_cache(maxsize=None)
def operands(case, K, N, T):
    """Seeded CPU operands: x [R, K] / sqrt(K) (the tail rows random too: nothing may read them into a result),
    w [E, N, K], dy [R, N] / sqrt(N), prev fp32 [E, N, K], and the offsets list."""
    rows, R = CASES[case]
    g = torch.Generator().manual_seed(1000 * K + N)
    x = (torch.randn(R, K, generator=g) / math.sqrt(K)).to(T)
    w = torch.randn(len(rows), N, K, generator=g).to(T)
    dy = (torch.randn(R, N, generator=g) / math.sqrt(N)).to(T)
    prev = torch.randn(len(rows), N, K, generator=g)
    return x, w, dy, prev, _offsets(rows)


def run(case, K, N, T, main_grad=False, backward=True):
    from apex.ops import grouped_linear

    x, w, dy, prev, off = operands(case, K, N, T)
    xd, wd = x.cuda().requires_grad_(), w.cuda().requires_grad_()
    if main_grad:
        wd.main_grad = prev.cuda()
    y = grouped_linear(xd, wd, torch.tensor(off, dtype=torch.int32, device="cuda"))
    if backward:
        y.backward(dy.cuda())
    return y.detach(), xd.grad, (wd.main_grad if main_grad else wd.grad)


@pytest.mark.parametrize("T", DTYPES, **ids)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case", list(CASES))
def test_forward(case, K, N, T):
    x, w, _, _, off = operands(case, K, N, T)
    y, _, _ = run(case, K, N, T, backward=False)
    assert y.shape == (x.shape[0], N) and y.dtype == T
    for e in range(w.shape[0]):
        acc, cond = acc_ref(x[off[e]:off[e + 1]], w[e])
        ref, bound = expected("none", T, K, acc, cond)["C"]
        check(y[off[e]:off[e + 1]], ref, bound, f"{case} K{K} N{N} expert {e}")
    assert not y[off[-1]:].any()   # tail rows: exactly zero


@pytest.mark.parametrize("main_grad", [False, True])
@pytest.mark.parametrize("T", DTYPES, **ids)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_backward(K, N, T, main_grad):
    x, w, dy, prev, off = operands("tail", K, N, T)
    _, dx, dw = run("tail", K, N, T, main_grad)
    assert dx.dtype == T and dw.dtype == (F32 if main_grad else T)
    for e in range(w.shape[0]):
        seg = slice(off[e], off[e + 1])
        acc, cond = acc_ref(dy[seg], w[e].t())            # the contraction runs over N
        ref, bound = expected("none", T, N, acc, cond)["C"]
        check(dx[seg], ref, bound, f"dx K{K} N{N} expert {e}")
        if off[e] == off[e + 1]:                          # the empty expert: zero, or main_grad bit-unchanged
            assert torch.equal(dw[e].cpu(), prev[e]) if main_grad else not dw[e].any()
            continue
        ref, bound = wgrad_expected(dy[seg], x[seg], 1, F32 if main_grad else T, prev[e] if main_grad else None)
        check(dw[e], ref, bound, f"dw K{K} N{N} expert {e} main_grad={main_grad}")
    assert not dx[off[-1]:].any()


def test_graph_capture_follows_offsets():
    """Forward + backward captured once, replayed with other segment boundaries in the same device table: bit-equal
    to an eager run (anything that read offsets on the host would have frozen the first boundaries, or failed
    the capture)."""
    from apex.ops import grouped_linear

    x, w, dy, _, off = operands("tail", 64, 256, BF16)
    xs, ws, dys = x.cuda().requires_grad_(), w.cuda().requires_grad_(), dy.cuda()
    offs = torch.tensor(off, dtype=torch.int32, device="cuda")

    def step():
        y = grouped_linear(xs, ws, offs)
        return (y,) + torch.autograd.grad(y, [xs, ws], dys)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for other in ([0, 128, 384, 384, 640, 960], [0, 0, 64, 512, 512, 576], off):
        offs.copy_(torch.tensor(other, dtype=torch.int32))
        graph.replay()
        got = [o.clone() for o in outs]
        for g, r in zip(got, step()):
            assert torch.equal(g, r), other


@pytest.mark.parametrize("T", DTYPES, **ids)
def test_declined_shape_takes_the_torch_path(T):
    from apex.ops import grouped_gemm_supported, grouped_linear

    rows, R = CASES["tail"]
    off, K, N = _offsets(rows), 96, 256
    assert not grouped_gemm_supported(R, K, N, len(rows))
    g = torch.Generator().manual_seed(96)
    x = (torch.randn(R, K, generator=g) / math.sqrt(K)).to(T)
    w = torch.randn(len(rows), N, K, generator=g).to(T)
    y = grouped_linear(x.cuda(), w.cuda(), torch.tensor(off, dtype=torch.int32, device="cuda"))
    for e in range(len(rows)):
        acc, cond = acc_ref(x[off[e]:off[e + 1]], w[e])
        ref, bound = expected("none", T, K, acc, cond)["C"]
        check(y[off[e]:off[e + 1]], ref, bound, f"K96 expert {e}")
    assert not y[off[-1]:].any()
