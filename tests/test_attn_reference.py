"""tests/attn_reference.py checked on the CPU: the fp32 emulation of the flash-attention kernels (the correct
implementation the bound has to admit) is inside the per-element bound on every case of the shared table and
every dtype, and not far inside it; the constants of the bound are pinned; each mutant of the emulation — a
way these kernels can be subtly wrong — is rejected on at least one case of its class in every dtype it exists
in, on inputs the correct emulation passes; the NumPy keep mask equals the scalar Python stream; and the exact
cases are exactly representable and tell every key apart. Every test prints its figures before asserting.
"""
import functools

import pytest
import torch

import attn_reference as R

F32, F16, BF16 = R.F32, R.F16, R.BF16
CASES = R.all_cases()
BY_NAME = {c.name: c for c in CASES}
# the worst ratio of the emulation over the whole table must reach FLOOR for every output in every dtype
# (dsum exists in the 16-bit units only): a bound looser than that proves nothing
FLOOR = 0.25


@functools.lru_cache(maxsize=None)
def _ops(name, T):
    return R.operands(BY_NAME[name], T)


def _ratios(name, T, mut=None):
    c = BY_NAME[name]
    ops = _ops(name, T)
    E = R.emulate(ops, T, c.p, mut)
    ref = R.reference(ops, *R.emu_stored(E))
    rr = R.ratios(E, ref, R.bounds(ref, ops, T))
    if c.dsum and T != F32 and mut is None:
        grads = [E[n].permute(0, 2, 1, 3) for n in ("dQ", "dK", "dV")]
        rr["dsum"] = R.ratio(R.emu_dsum(*grads), *R.dsum_expected(*grads))[0]
    return rr


@functools.lru_cache(maxsize=None)
def _table():
    """{(case, dtype): {output: worst ratio}} of the unmutated emulation."""
    return {(c.name, T): _ratios(c.name, T) for c in CASES for T in c.dtypes}


def test_constants_pinned():
    assert R.HALF_ULP == {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}
    assert R.TINY == {F32: 2.0 ** -149, F16: 2.0 ** -24, BF16: 2.0 ** -133}
    assert R.P_TINY == {F32: 2.0 ** -126, F16: 2.0 ** -24, BF16: 2.0 ** -126}
    assert (R.E23, R.E24, R.BWD_BK) == (2.0 ** -23, 2.0 ** -24, 128)
    assert R.FTZ32 == 2.0 ** -126
    assert R.FWD_TILE == {BF16: 64, F16: 64, F32: 32}
    assert abs(R.LOG2E * R.LN2 - 1.0) < 1e-15
    assert [R.drop_thresh(p) for p in (0.0, 0.001, 0.1, 0.5, 0.9, 0.999)] == [0, 1, 26, 128, 230, 255]
    assert len(R.MUTANTS) == 16 and len(R.MUTANTS) - len(R.MUTANTS_16BIT_ONLY) >= 12
    assert R.MUT_EPS == {BF16: 2.0 ** -5, F16: 2.0 ** -8, F32: 2.0 ** -21}


def test_case_table_shapes():
    """The table holds the shapes at which these kernels change path: every boundary key length, the query counts independent of
    them, B <= 2, H <= 3 (one grouped case with four heads), S <= 320, a non-power-of-two B * H."""
    sks, sqs = {c.Sk for c in CASES}, {c.Sq for c in CASES}
    assert set(R.SK_SHORT + R.SK_LONG) <= sks and set(R.SQS) <= sqs
    assert sum(1 for c in CASES if c.Sq != c.Sk and c.Sq in R.SQS) >= 4
    assert all(c.B <= 2 and c.Sq <= 320 and c.Sk <= 320 for c in CASES)
    assert [c.name for c in CASES if c.H > 3] == ["gqa-g2"]
    assert any(c.B * c.H == 6 for c in CASES)
    assert len({c.name for c in CASES}) == len(CASES)
    for need in ((160, 96), (40, 200)):
        assert any((c.Sq, c.Sk) == need for c in CASES)
    assert any(c.k_lens and 0 in c.k_lens for c in CASES) and any(c.k_lens and 1 in c.k_lens for c in CASES)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_emulation_inside_bound(name):
    for T in BY_NAME[name].dtypes:
        rr = _table()[(name, T)]
        print(f"{name} {R.DT_NAME[T]}: " + " ".join(f"{k} {v:.3f}" for k, v in rr.items()))
        for k, v in rr.items():
            assert v <= 1.0, (name, R.DT_NAME[T], k, v)


def test_bound_is_not_loose():
    worst = {}
    for (name, T), rr in _table().items():
        for k, v in rr.items():
            key = (k, R.DT_NAME[T])
            if v > worst.get(key, (-1.0, ""))[0]:
                worst[key] = (v, name)
    print("fp32 emulation, worst |got - ref| / bound per output and dtype:")
    for key in sorted(worst):
        print(f"  {key[0]} {key[1]}: {worst[key][0]:.3f}  ({worst[key][1]})")
    assert {k[0] for k in worst} == set(R.OUTPUTS) | {"dsum"}
    low = {k: v for k, v in worst.items() if v[0] < FLOOR}
    assert not low, low


@pytest.mark.parametrize("mut", list(R.MUTANTS))
def test_mutant_rejected(mut):
    """Rejected (worst ratio > 1 on some output) by at least one case of its class in every dtype in which the
    mutation exists; the unmutated emulation passes the same case."""
    for T in R.DTYPES:
        if T == F32 and mut in R.MUTANTS_16BIT_ONLY:
            continue
        cands = [c for c in CASES if T in c.dtypes and R.MUTANTS[mut](c, T)]
        assert cands, (mut, R.DT_NAME[T])
        hit = None
        for c in sorted(cands, key=lambda c: c.B * c.H * c.Sq * c.Sk):
            rr = _ratios(c.name, T, mut)
            top = max(rr.values())
            if top > 1.0:
                assert max(_table()[(c.name, T)].values()) <= 1.0
                hit = (c.name, top, max(rr, key=rr.get))
                break
        print(f"{mut} {R.DT_NAME[T]}: {len(cands)} cases in class, rejected by {hit}")
        assert hit is not None, (mut, R.DT_NAME[T])


def test_unrounded_p_is_not_rejectable():
    """Leaving P unrounded before the PV product only removes a rounding: it stays inside the bound on every
    case (which is why it is not among the mutants)."""
    top = max(max(_ratios(c.name, T, "p_unrounded").values()) for c in CASES[::4] for T in c.dtypes if T != F32)
    print(f"p_unrounded: worst ratio {top:.3f}")
    assert top <= 1.0


@pytest.mark.parametrize("Sq,Sk,thresh", [(37, 100, 26), (5, 33, 128), (3, 257, 230)])
def test_numpy_keep_mask_equals_python_stream(Sq, Sk, thresh):
    from test_attention_ext_gpu import _keep_bits_python

    seed, offset, BH = 0x1234_5678_9ABC, 0x7777_0000_0011, 3
    got = R.keep_mask(seed, offset, BH, Sq, Sk, thresh)
    assert got.shape == (BH, Sq, Sk)
    rows = [(b, r) for b in range(BH) for r in range(Sq)]
    for b, r in rows[:: max(1, len(rows) // 40)] + [rows[-1]]:
        assert got[b, r].astype(int).tolist() == _keep_bits_python(seed, offset, b, r, Sq, Sk, thresh), (b, r)
    rate = float(got.mean())
    print(f"Sq {Sq} Sk {Sk} thresh {thresh}: keep rate {rate:.4f} (expected {1 - thresh / 256:.4f})")
    assert abs(rate - (1 - thresh / 256)) < 0.05


def _exact_in(x, T):
    return torch.equal(x.to(T).double(), x.double())


@pytest.mark.parametrize("shape", R.UNIFORM_SHAPES, ids=str)
def test_uniform_exact_case(shape):
    Sq, Sk, n, D = shape
    keep = torch.from_numpy(R.keep_mask(11, 22, 2 * 3, Sq, Sk, 128)).view(2, 3, Sq, Sk)
    for kp in (None, keep):
        for T in (BF16, F16, F32):
            ops, exp = R.uniform_operands(2, 3, Sq, Sk, n, D, T, kp)
            assert _exact_in(exp["O"], T) and _exact_in(exp["dV"], T), (shape, T)
            ref = R.reference(ops)
            assert torch.equal(ref.O.permute(0, 2, 1, 3), exp["O"].double())
            assert float((ref.dV.permute(0, 2, 1, 3) - exp["dV"].double()).abs().max()) < 1e-12
            assert float((ref.lse[ref.lse < R.INF] - exp["lse"]).abs().max()) < 1e-12 if kp is None else True
        # every visible key changes the expected output when removed or duplicated: its V row is not zero, and
        # no two keys carry the same row
        v = ops.v[0, :n, 0].double()
        assert bool((v.abs().sum(-1) > 0).all()) and len(torch.unique(v, dim=0)) == n
        w = torch.ones(n, dtype=torch.float64)
        base = w @ v
        for key in (0, n // 2, n - 1):
            for f in (0.0, 2.0):
                w2 = w.clone()
                w2[key] = f
                assert not torch.equal(w2 @ v, base)


@pytest.mark.parametrize("shape", R.ONEHOT_SHAPES, ids=str)
def test_onehot_exact_case(shape):
    Sq, Sk, D, causal = shape
    for T in (BF16, F16, F32):
        ops, exp = R.onehot_operands(2, 3, Sq, Sk, D, T, causal)
        assert _exact_in(exp["O"], T) and _exact_in(exp["dV"], T)
        ref = R.reference(ops)
        assert torch.equal(ref.O.permute(0, 2, 1, 3), exp["O"].double())
        assert torch.equal(ref.dV.permute(0, 2, 1, 3), exp["dV"].double())
        assert float(ref.lse.abs().max()) == 0.0 and float(ref.dK.abs().max()) == 0.0 and float(ref.dQ.abs().max()) == 0.0
        pi = exp["pi"]
        assert bool((pi <= torch.arange(Sq)).all()) or not causal
        # no two keys of a head carry the same V row: a query that read another key has another output
        for h in range(3):
            assert len(torch.unique(ops.v[0, :, h].double(), dim=0)) == Sk
