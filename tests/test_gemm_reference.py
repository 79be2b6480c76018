"""tests/gemm_reference.py checked on the CPU: the fp32 emulation of every GEMM epilogue (the correct
implementation the bound has to admit) is inside the per-element bound on every case of the shared
table; the constants of the bound are pinned; and each mutant of the emulation — a way these kernels
can be subtly wrong — is rejected on at least one case of the class it belongs to, on inputs the
correct emulation passes. Every test prints its figures before asserting; the worst error / bound
of the emulation per epilogue, output and dtype is printed at the end.
"""
import functools
import math

import pytest
import torch

import gemm_reference as R

F32, F16, BF16 = R.F32, R.F16, R.BF16
NT_IDS = [s.name for s in R.NT_SHAPES]


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    R.WORST.clear()
    yield
    print("\nfp32 emulation, worst |got - ref| / bound per epilogue, output and dtype:")
    for tag in sorted(R.WORST):
        print(f"  {tag}: {R.WORST[tag][0]:.3f}  ({R.WORST[tag][1]})")


@functools.lru_cache(maxsize=None)
def _case(shape, T):
    A, B, bias, aux = R.dense_operands(shape.name, shape.M, shape.N, shape.K, T)
    acc, cond = R.acc_ref(A, B)
    return A, B, bias, aux, acc, cond


def _bdts(epi, T):
    return (F32, T) if R.colsum(epi) else (None,)


def _emu_ratio(shape, T, epi, bdt, mut=None, worst=None, tag=None):
    A, B, bias, aux, acc, cond = _case(shape, T)
    c, x = R.emu_gemm(epi, T, A, B, bias, aux, bdt, mut)
    return R.check_epilogue(epi, T, shape.K, acc, cond, c, x, bias, aux, bdt, what=f"{shape.name} {R.DT_NAME[T]}",
                            tag=tag, worst=worst)


def test_constants_pinned():
    assert R.HALF_ULP == {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}
    assert R.TINY == {F32: 2.0 ** -149, F16: 2.0 ** -24, BF16: 2.0 ** -133}
    assert (R.E23, R.E24, R.BK, R.S2) == (2.0 ** -23, 2.0 ** -24, 64, 2.0)
    assert R.E_PHI == 0.75e-7 + 10 * 2.0 ** -24 and R.E_SIG == 6 * 2.0 ** -24
    assert len(R.EPIS) == 10 and len(R.MUTANTS) + len(R.WGRAD_MUTANTS) == 14
    # the activation terms stay far below one rounding of the output wherever the output is of order 1
    assert 8 * R.E_PHI < R.HALF_ULP[F16] / 32


def test_second_derivative_bound():
    """S2 bounds |gelu''| and |gelu'''| of both forms (central differences of the closed forms on a grid), and
    the closed-form derivatives agree with differences of the functions they derive."""
    x = torch.linspace(-12.0, 12.0, 240001, dtype=torch.float64)
    h = 1e-4
    for tanh in (False, True):
        d1 = (R.gelu64(x + h, tanh) - R.gelu64(x - h, tanh)) / (2 * h)
        d2 = (R.dgelu64(x + h, tanh) - R.dgelu64(x - h, tanh)) / (2 * h)
        d3 = (R.d2gelu64(x + h, tanh) - R.d2gelu64(x - h, tanh)) / (2 * h)
        e1, e2 = float((d1 - R.dgelu64(x, tanh)).abs().max()), float((d2 - R.d2gelu64(x, tanh)).abs().max())
        s2, s3 = float(R.d2gelu64(x, tanh).abs().max()), float(d3.abs().max())
        print(f"tanh={tanh}: sup|gelu''| {s2:.4f}, sup|gelu'''| {s3:.4f}; closed forms vs differences {e1:.2e} {e2:.2e}")
        assert e1 < 1e-7 and e2 < 1e-7
        assert s2 <= R.S2 and s3 <= R.S2
    # the two forms differ by a few 1e-4: what a swapped epilogue has to be caught on
    d = (R.gelu64(x, True) - R.gelu64(x, False)).abs().max()
    assert 1e-4 < float(d) < 1e-3


def test_activation_emulation_within_e_act():
    """The kernel's polynomial / sigmoid formulas in fp32 are within E_act and E_g of the float64 functions."""
    x = torch.cat([torch.linspace(-12.0, 12.0, 200001), torch.randn(100000, generator=R._gen("act")) * 2.0]).float()
    for tanh in (False, True):
        y, g = R.emu_gelu_and_grad(x, tanh)
        xd = x.double()
        ry = float(((y.double() - R.gelu64(xd, tanh)).abs() / R.e_act(xd, tanh).clamp(min=1e-300)).max())
        rg = float(((g.double() - R.dgelu64(xd, tanh)).abs() / R.e_g(xd, tanh)).max())
        print(f"tanh={tanh}: fp32 formula error / E_act {ry:.3f}, / E_g {rg:.3f}")
        assert ry <= 1.0 and rg <= 1.0


def _n_unique_rows(a):
    """Number of distinct rows of an int64 matrix, counted on three seeded random projections of each row
    (equal rows project alike, so this never overcounts; three 40-bit projections do not collide by chance)."""
    w = torch.randint(1, 1 << 20, (a.shape[1], 3), generator=R._gen("rows"))
    return len(torch.unique(a.double() @ w.double(), dim=0))   # (below 2**53: exact in float64)


def _exact_shapes():
    """(M, N, K) of every exact case the GPU file runs: the NT tables, the persistent shapes of 256 CUs, the weight-gradient shapes (P, Q, R)."""
    out = {(s.M, s.N, s.K) for s in R.NT_SHAPES + R.LAYOUT}
    out |= {(s.M, s.N, s.K) for i, s in enumerate(R.persist_shapes(256)) if i in (1, 3)}   # (those with exact cases)
    out |= {(p, q, r) for (p, q) in R.WGRAD_PQ for r in (192, 448)}
    return sorted(out)


def test_exact_operands_tell_every_position_apart():
    """For every exact shape: C is a distinct function of (m, n) — all rows differ, so every 8-, 64-, 128- and
    256-row block differs from every other, and all columns differ where 64 rows tell them apart — every
    K-tile of A and of B carries nonzeros, every row of A has its eight, and nothing exceeds 256."""
    for M, N, K in _exact_shapes():
        A, B, bias, aux = R.exact_operands(M, N, K)
        acc = R.exact_acc(A, B)
        rows, cols = _n_unique_rows(acc), _n_unique_rows(acc.t().contiguous())
        print(f"{M}x{N}x{K}: {rows} distinct rows, {cols} distinct columns, max |acc| {int(acc.abs().max())}")
        assert rows == M, (M, N, K)
        assert cols == N or M < 64, (M, N, K)
        for blk in (8, 64, 128, 256):      # neighbouring blocks, compared outright
            for r0 in range(0, min(M, 1024) - 2 * blk + 1, blk):
                assert not torch.equal(acc[r0:r0 + blk], acc[r0 + blk:r0 + 2 * blk]), (M, N, K, blk, r0)
        for c0 in range(0, N - 15, 8):
            assert M < 64 or not torch.equal(acc[:, c0:c0 + 8], acc[:, c0 + 8:c0 + 16]), (M, N, K, c0)
        assert bool(((A != 0).sum(1) == R.EXACT_NNZ).all())
        for t in range(K // 64):
            assert int((A[:, t * 64:(t + 1) * 64] != 0).sum()) > 0, (M, N, K, "A", t)
            assert int((B[:, t * 64:(t + 1) * 64] != 0).sum()) > 0, (M, N, K, "B", t)
        assert int(acc.abs().max()) <= 128 and int(bias.abs().max()) <= 8 and int(aux.abs().max()) <= 2
        assert 2 * 128 * M <= 2 ** 24                      # a column of |acc * aux| sums exactly in fp32


def test_exact_operands():
    """The gathered product is the int64 matrix product, and the emulation reproduces the integer cases bit
    for bit."""
    for M, N, K in [(256, 256, 64), (300, 200, 192), (77, 8, 128), (512, 768, 320), (1, 264, 64), (8, 1608, 448)]:
        A, B, bias, aux = R.exact_operands(M, N, K)
        assert torch.equal(R.exact_acc(A, B), A @ B.t())
        for T in R.DTYPES:
            At, Bt, bt, xt = A.to(T), B.to(T), bias.to(T), aux.to(T)
            for epi in R.EXACT_EPIS:
                c, x = R.emu_gemm(epi, T, At, Bt, bt, xt, F32 if epi == "mul" else None)
                for name, v in R.exact_expected(epi, A, B, bias, aux).items():
                    got = c if name == "C" else x
                    assert torch.equal(got.double(), v.double()), (M, N, K, epi, name)


@pytest.mark.parametrize("T", R.DTYPES, ids=lambda t: R.DT_NAME[t])
@pytest.mark.parametrize("shape", R.NT_SHAPES, ids=NT_IDS)
def test_emulation_within_bound(shape, T):
    for epi in R.EPIS:
        for bdt in _bdts(epi, T):
            r = _emu_ratio(shape, T, epi, bdt, tag="emu")
            print(f"{shape.name} {R.DT_NAME[T]} {epi} db={R.DT_NAME[bdt]}: worst error / bound {r:.3f}")


def _class_cases(pred):
    for shape in R.NT_SHAPES:
        if shape.M * shape.N > 600 * 600 or shape.K > 320:
            continue  # (the small shapes of each class are enough, and quick)
        for T in R.DTYPES:
            for epi in R.EPIS:
                if pred(epi, T, shape.M, shape.N, shape.K):
                    yield shape, T, epi


@pytest.mark.parametrize("mut", sorted(R.MUTANTS))
def test_mutant_rejected(mut):
    """The mutant is outside the bound on at least one case of its class; the correct emulation is inside it
    on every case looked at."""
    rejected, seen = [], 0
    for shape, T, epi in _class_cases(R.MUTANTS[mut]):
        bdt = F32 if R.colsum(epi) else None
        ok = _emu_ratio(shape, T, epi, bdt, worst={})
        assert ok <= 1.0, (shape.name, epi, ok)
        bad = _emu_ratio(shape, T, epi, bdt, mut=mut, worst={})
        seen += 1
        if bad > 1.0:
            rejected.append((shape.name, R.DT_NAME[T], epi, round(bad, 2), round(ok, 3)))
        if len(rejected) >= 3:
            break
    print(f"{mut}: {seen} cases tried, rejected on (case, dtype, epilogue, mutant ratio, correct ratio): {rejected}")
    assert seen > 0 and rejected, mut


# ----------------------------------------------------------------------------
# weight-gradient form
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("T", R.DTYPES, ids=lambda t: R.DT_NAME[t])
def test_wgrad_emulation_within_bound(T):
    for (Rr, P, Q, s) in R.WGRAD:
        A, B = R.dense_wgrad_operands(f"{Rr}x{P}x{Q}", Rr, P, Q, T)
        for odt in (F32, T):
            ref, bound = R.wgrad_expected(A, B, s, odt)
            r = R.check(R.emu_wgrad(A, B, s, odt), ref, bound, f"wgrad {Rr}x{P}x{Q} s{s}", f"emu wgrad {R.DT_NAME[T]}->{R.DT_NAME[odt]}")
        prev = torch.randn(P, Q, generator=R._gen("prev"))
        ref, bound = R.wgrad_expected(A, B, 1, F32, prev)
        R.check(R.emu_wgrad(A, B, 1, F32, prev), ref, bound, f"wgrad_acc {Rr}x{P}x{Q}", f"emu wgrad_acc {R.DT_NAME[T]}")
    assert all(Rr // 64 >= s for (Rr, _, _, s) in R.WGRAD) and len(R.WGRAD) == 36


@pytest.mark.parametrize("mut", R.WGRAD_MUTANTS)
def test_wgrad_mutant_rejected(mut):
    rejected, seen = [], 0
    for (Rr, P, Q, s) in R.WGRAD:
        if s == 1:
            continue
        for T in R.DTYPES:
            A, B = R.dense_wgrad_operands(f"{Rr}x{P}x{Q}", Rr, P, Q, T)
            ref, bound = R.wgrad_expected(A, B, s, F32)
            ok = R.ratio(R.emu_wgrad(A, B, s, F32), ref, bound)[0]
            bad = R.ratio(R.emu_wgrad(A, B, s, F32, mut=mut), ref, bound)[0]
            assert ok <= 1.0
            seen += 1
            if bad > 1.0:
                rejected.append((Rr, P, Q, s, R.DT_NAME[T], round(bad, 1)))
    print(f"{mut}: rejected on {len(rejected)} of {seen} cases")
    assert seen and len(rejected) == seen, (mut, rejected)


def test_wgrad_exact():
    for (P, Q) in R.WGRAD_PQ:
        A, B, _, _ = R.exact_operands(P, Q, 192)
        for T in R.DTYPES:
            a, b = A.t().contiguous().to(T), B.t().contiguous().to(T)
            for s, odt in ((1, T), (3, F32), (3, T)):
                assert torch.equal(R.emu_wgrad(a, b, s, odt).double(), R.exact_acc(A, B).double())


def test_case_tables():
    """The shapes the issue names are in the tables, and the persistent shapes follow the CU count."""
    assert {(s.M, s.N, s.K) for s in R.FULL} >= {(256, 256, k) for k in (64, 128, 192, 256, 320)} | {
        (512, 768, 128), (2304, 512, 64), (256, 512, 1024)}
    assert {s.M for s in R.EDGE} == {1, 77, 129, 255, 257, 300} and {s.N for s in R.EDGE} == {8, 72, 200, 264, 520}
    assert {s.K for s in R.EDGE} == {64, 128, 192, 1024} and (300, 200, 1024) in {(s.M, s.N, s.K) for s in R.EDGE}
    for cus in (256, 304, 64):
        two, three = R.persist_shapes(cus)[0], R.persist_shapes(cus)[-1]
        assert (two.M // 256) * (two.N // 256) == 4 * (cus // 4) + 8 > cus
        assert (three.M // 256) * (three.N // 256) > 2 * (cus // 8) * 8 and three.epis == ("none", "bias_gelu_d", "mul")
    assert math.isclose(R.GELU_C, 0.7978845608028654)
