"""Transposed-read weight-gradient GEMM (csrc/gemm.hip gemm_tt / gemm_tt_acc / gemm_tt_f8): the LDS staging
addresses — a loop-invariant per-lane offset plus a wave-uniform 64-bit base advanced per K-tile.

Exactness instead of a tolerance: the operands are small integers, the output is fp32 and R <= 4096, so
every partial sum stays below 2^24 and the fp32 reference is exact in any summation order. A mis-staged
K-row or 16-byte chunk shows as a nonzero difference.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _C():
    import apex._ext as e

    return e.require()


def _ints(R, C, dt, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randint(-2, 3, (R, C), device=DEV, generator=g).to(dt)


def _check(R, P, Q, splits, dt):
    C = _C()
    dy = _ints(R, P, dt, 1000 * R + P)
    x = _ints(R, Q, dt, 1000 * R + Q + 1)
    assert C.gemm_tt_supported(dy, x, splits)
    out = C.gemm_tt(dy, x, splits, torch.float32)
    assert out.shape == (P, Q) and out.dtype == torch.float32
    torch.testing.assert_close(out, dy.float().t() @ x.float(), rtol=0, atol=0)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("R", [64, 128, 192, 320])
def test_k_tile_counts(R, dt):
    """1, 2, 3 and 5 K-tiles: the prologue alone, the first A(t+1) / B(t+2) advance, the odd tail tile of
    the two-tile loop body, the steady state."""
    _check(R, 256, 256, 1, dt)


@pytest.mark.parametrize("R,P,Q", [(192, 768, 512), (128, 4800, 1600)])
def test_tile_origins_and_unequal_ld(R, P, Q):
    """Nonzero tile origins in both operands and lda != ldb."""
    _check(R, P, Q, 1, torch.bfloat16)


@pytest.mark.parametrize("R,splits", [(448, 3), (320, 5)])
def test_uneven_slices(R, splits):
    """Slices of 2-3 K-tiles and of one K-tile: the slice base is not a multiple of the slice length."""
    _check(R, 256, 256, splits, torch.bfloat16)


@pytest.mark.parametrize("R,P,Q", [(512, 200, 264), (128, 8, 1608)])
def test_clamped_partial_tiles(R, P, Q):
    """Chunks past the last row read the last full chunk (the clamp is part of the per-lane offset)."""
    _check(R, P, Q, 1, torch.bfloat16)


def test_gemm_tt_acc():
    """The fp32 accumulating epilogue at 3 K-tiles on a partial-tile shape: exact sum onto the previous
    contents, the guard band after the accumulator untouched."""
    C = _C()
    R, P, Q = 192, 1600, 488
    dy = _ints(R, P, torch.bfloat16, 11)
    x = _ints(R, Q, torch.bfloat16, 12)
    buf = torch.full((P * Q + 256,), 5.0, device=DEV)
    mg = buf[:P * Q].view(P, Q)
    mg.copy_(_ints(P, Q, torch.float32, 13))
    before = mg.clone()
    C.gemm_tt_acc(dy, x, mg)
    torch.testing.assert_close(mg, before + dy.float().t() @ x.float(), rtol=0, atol=0)
    assert (buf[P * Q:] == 5.0).all()


@pytest.mark.parametrize("fmt_a", [1, 0])  # dY codes: e5m2 / e4m3 (integers in [-2, 2] are exact in both)
@pytest.mark.parametrize("R,P,Q,splits", [(128, 256, 256, 1), (256, 256, 256, 1), (384, 256, 256, 1),
                                          (640, 256, 256, 3)])
def test_gemm_tt_f8(R, P, Q, splits, fmt_a):
    """fp8: 128-row K-tiles, pieces of four K-rows; 1, 2 and 3 K-tiles and uneven slices (1, 2, 2)."""
    C = _C()
    dta = torch.float8_e5m2 if fmt_a == 1 else torch.float8_e4m3fn
    dy = _ints(R, P, torch.float32, 21 + R)
    x = _ints(R, Q, torch.float32, 22 + R)
    a8 = dy.to(dta).view(torch.uint8)
    b8 = x.to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(a8.view(dta).float(), dy) and torch.equal(b8.view(torch.float8_e4m3fn).float(), x)
    assert C.gemm_tt_f8_supported(a8, b8, splits)
    one = torch.ones(1, device=DEV)
    out = C.gemm_tt_f8(a8, b8, one, one, fmt_a, 0, splits, torch.float32)
    torch.testing.assert_close(out, dy.t() @ x, rtol=0, atol=0)


@pytest.fixture(scope="module")
def big_operands():
    """dY [589824, 4096] bf16 (4.8 GB), zero except its last 256 rows; X [589824, 256] small integers; the
    exact reference from those 256 rows."""
    R, P, Q = 589824, 4096, 256
    try:
        dy = torch.zeros(R, P, device=DEV, dtype=torch.bfloat16)
        x = _ints(R, Q, torch.bfloat16, 31)
    except torch.cuda.OutOfMemoryError:
        pytest.skip("not enough device memory for a 4.8 GB operand")
    dy[-256:] = _ints(256, P, torch.bfloat16, 32)
    ref = dy[-256:].float().t() @ x[-256:].float()
    yield dy, x, ref
    del dy, x
    torch.cuda.empty_cache()


@pytest.mark.parametrize("splits", [1, 9])
def test_operand_past_4gib(big_operands, splits):
    """splits = 1: one workgroup's running base crosses 2^32 bytes inside its K loop; splits = 9: the last
    slice's base lies past 2^32. Nothing in the address may be a 32-bit running value."""
    C = _C()
    dy, x, ref = big_operands
    assert dy.numel() * dy.element_size() > 2 ** 32
    out = C.gemm_tt(dy, x, splits, torch.float32)
    torch.testing.assert_close(out, ref, rtol=0, atol=0)
