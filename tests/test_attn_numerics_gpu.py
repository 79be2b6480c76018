"""Flash attention on the GPU against tests/attn_reference.py: every forward loop, both backward schemes, the
fp32 unit and the group reduce, bf16 / fp16 / fp32, held element by element to the derived bound of the float64
reference (dense cases), to bit equality (exact cases), to untouched guard bands around caller-provided
gradients, and to the NumPy keep mask on the whole tensor; plus the binding's refusals, the empty shapes and
the wrappers' fallbacks. Every test prints its figures before asserting; the module fixture prints the worst
error / bound per path, output and dtype (committed as profiles/attention_numerics_worst.txt).

Worst error / bound of the run that produced the committed table: see that file.
"""
import functools
import math

import pytest
import torch

import attn_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16, BF16 = R.F32, R.F16, R.BF16
CASES = R.all_cases()
BY_NAME = {c.name: c for c in CASES}
CASE_IDS = [f"{c.name}-{R.DT_NAME[T]}" for c in CASES for T in c.dtypes]
CASE_ARGS = [(c.name, T) for c in CASES for T in c.dtypes]


@functools.lru_cache(maxsize=None)
def _C():
    import apex._ext as e

    C = e.require()
    # the refusal tests below must never meet a binding without the device / shape checks: the two path helpers
    # were added together with them
    assert hasattr(C, "attn_fwd_loop") and hasattr(C, "attn_bwd_two_kernel")
    return C


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    R.WORST.clear()
    yield
    print("\n== attention numerics: worst |got - ref| / bound per path, output and dtype ==")
    for tag in sorted(R.WORST):
        print(f"  {tag}: {R.WORST[tag][0]:.3f}  ({R.WORST[tag][1]})")
    print("== end ==")


def _native_d(D):
    return next(n for n in (32, 64, 128, 256) if D <= n)


def _paths(case, T):
    """(forward path, backward path) names of a case."""
    if T == F32:
        return "f32", "f32"
    C = _C()
    fwd = C.attn_fwd_loop(_native_d(case.D), case.Sk, case.p > 0, case.bias != "none")
    return fwd, "two_kernel" if C.attn_bwd_two_kernel(case.Sk) else "fused"


def _strided(t):
    """t's values in a view of a wider buffer: gaps on the sequence, head and dim axes, 16-byte aligned."""
    B, S, H, D = t.shape
    buf = torch.full((B, S + 2, H + 1, D + 16), 3.0, dtype=t.dtype, device=t.device)
    view = buf[:, 1:S + 1, 1:, 8:8 + D]
    view.copy_(t)
    return view


def _device_operands(case, ops):
    """(q, k, v, do, holders of the gradients) on the device in the case's layout."""
    dev = torch.device(DEV)
    q, k, v, do = (t.to(dev) for t in (ops.q, ops.k, ops.v, ops.do))
    if case.layout == "packed":
        qkv = torch.stack([q, k, v], 2)
        q, k, v = qkv.unbind(2)
        dq, dk, dv = torch.empty_like(qkv).unbind(2)
    elif case.layout == "gpacked":
        qkv = torch.cat([q, k, v], 2)
        H, Hk = case.H, case.Hk
        q, k, v = qkv[:, :, :H], qkv[:, :, H:H + Hk], qkv[:, :, H + Hk:]
        d = torch.empty_like(qkv)
        dq, dk, dv = d[:, :, :H], d[:, :, H:H + Hk], d[:, :, H + Hk:]
    elif case.layout == "strided":
        q, k, v, do = (_strided(t) for t in (q, k, v, do))
        dq, dk, dv = (_strided(torch.zeros_like(t)) for t in (q, k, v))
    else:
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    return q, k, v, do, dq, dk, dv


def _run(case, T, ops):
    """The kernels on a case: {output: tensor in reference layout} plus the stored o / lse and dsum."""
    from apex.contrib.multihead_attn.attention import prepare_bias

    C = _C()
    dev = torch.device(DEV)
    q, k, v, do, dq, dk, dv = _device_operands(case, ops)
    bias = None if ops.bias is None else prepare_bias(ops.bias.to(dev), case.B, case.H, case.Sq, case.Sk, T)
    kl = None if case.k_lens is None else torch.tensor(case.k_lens, dtype=torch.int32, device=dev)
    seed, off = case.seed_offset if case.p > 0 else (0, 0)
    o, lse, dmask = C.flash_attn_fwd(q, k, v, case.causal, case.scale, case.p, seed, off, kl, bias)
    dbias = torch.zeros(bias.shape, dtype=torch.float32, device=dev) if case.trainable else None
    # (the bias-gradient column sums are a feature of the 16-bit units: the fp32 unit runs the same case without)
    dsum = torch.zeros(case.B, 3, case.H, case.D, dtype=torch.float32, device=dev) if case.dsum and T != F32 else None
    C.flash_attn_bwd(do, q, k, v, o, lse, dq, dk, dv, case.causal, case.scale, case.p, seed, off, kl, dmask, dsum, 0,
                     bias, dbias=dbias)
    torch.cuda.synchronize()
    got = {"O": R.bh(o), "lse": lse, "dQ": R.bh(dq), "dK": R.bh(dk), "dV": R.bh(dv), "dbias": dbias}
    return {n: (None if t is None else t.cpu()) for n, t in got.items()}, o.cpu(), lse.cpu(), dsum, (dq, dk, dv)


def _check_all(got, ref, bd, what, fwd, bwd, T):
    worst = {}
    for n in R.OUTPUTS:
        if got.get(n) is None or n not in bd:
            continue
        worst[n] = R.ratio(got[n], getattr(ref, n), bd[n])[0]
    print(f"{what} [{fwd} / {bwd}]: " + " ".join(f"{n} {x:.3f}" for n, x in worst.items()))
    for n in worst:
        path = fwd if n in ("O", "lse") else bwd
        R.check(got[n], getattr(ref, n), bd[n], f"{what} {n}", f"{path} {n} {R.DT_NAME[T]}")
    # rows with no visible key: exactly O = 0, lse = +inf, dQ = 0
    dead = ~ref.live.squeeze(-1)
    if bool(dead.any()):
        assert bool((got["O"].double()[dead] == 0).all()) and bool((got["lse"][dead] == R.INF).all()), what
        assert bool((got["dQ"].double()[dead] == 0).all()), what


@pytest.mark.parametrize("name,T", CASE_ARGS, ids=CASE_IDS)
def test_dense_case_inside_bound(name, T):
    case = BY_NAME[name]
    ops = R.operands(case, T)
    what = f"{name} {R.DT_NAME[T]}"
    fwd, bwd = _paths(case, T)
    if case.layout == "padded":
        return _padded_case(case, T, ops, what, fwd, bwd)
    got, o, lse, dsum, grads = _run(case, T, ops)
    ref = R.reference(ops, o, lse)
    _check_all(got, ref, R.bounds(ref, ops, T), what, fwd, bwd, T)
    if case.p > 0:    # the whole keep mask of the debug kernel against the NumPy stream
        seed, off = case.seed_offset
        m = _C().flash_dropout_mask(case.B, case.H, case.Sq, case.Sk, case.p, seed, off, torch.device(DEV)).cpu()
        assert torch.equal(m.bool(), ops.keep), what
    if dsum is not None:
        dref, dbound = R.dsum_expected(*(g.cpu() for g in grads))
        w = R.ratio(dsum.cpu(), dref, dbound)[0]
        print(f"{what} dsum {w:.3f}")
        R.check(dsum.cpu(), dref, dbound, f"{what} dsum", f"{bwd} dsum {R.DT_NAME[T]}")


def _padded_case(case, T, ops, what, fwd, bwd):
    """A head dim that is not native, through attention() and autograd (zero padding to the next native dim)."""
    from apex.contrib.multihead_attn.attention import attention

    q, k, v = (t.to(DEV).requires_grad_(True) for t in (ops.q, ops.k, ops.v))
    o = attention(q, k, v, None, 0.0, case.causal)
    o.backward(ops.do.to(DEV))
    got = {"O": R.bh(o.detach()).cpu(), "dQ": R.bh(q.grad).cpu(), "dK": R.bh(k.grad).cpu(), "dV": R.bh(v.grad).cpu()}
    ref = R.reference(ops, o.detach().cpu())
    pad = R.Ops(*(torch.nn.functional.pad(t, (0, _native_d(case.D) - case.D)) for t in (ops.q, ops.k, ops.v, ops.do)),
                ops.scale, ops.causal)
    refp = R.reference(pad, torch.nn.functional.pad(o.detach().cpu(), (0, _native_d(case.D) - case.D)))
    bd = {n: b[..., :case.D] if n != "lse" else b for n, b in R.bounds(refp, pad, T, stored="o").items()}
    _check_all(got, ref, bd, what, fwd, bwd, T)


def test_table_reaches_every_instantiation():
    """The dense table launches every forward instantiation attn_fwd_reaches allows (loop x D x causal x dropout x
    bias x 16-bit dtype), every 16-bit backward kernel x causal x dropout x bias x dsum x dtype, and the fp32
    unit's D x causal x dropout x bias."""
    C = _C()
    fwd_want, fwd_got, bwd_want, bwd_got, f32_want, f32_got = set(), set(), set(), set(), set(), set()
    flags = [(c, p, b) for c in (False, True) for p in (False, True) for b in (False, True)]
    for T in (BF16, F16):
        for D in (32, 64, 128, 256):
            for c, p, b in flags:
                for Sk in (128, 129):      # attn_fwd_reaches: the loops of the two key classes
                    fwd_want.add((C.attn_fwd_loop(D, Sk, p, b), D, c, p, b, T))
        for c, p, b in flags:
            for ds in (False, True):
                if not (b and ds):
                    bwd_want |= {(kern, c, p, b, ds, T) for kern in ("fused", "delta", "dkdv", "dq")}
    for D in (32, 64, 128):
        f32_want |= {(D, c, p, b) for c, p, b in flags}
    for case in CASES:
        for T in case.dtypes:
            key = (case.causal, case.p > 0, case.bias != "none")
            D = _native_d(case.D)
            if T == F32:
                f32_got.add((D,) + key)
                continue
            fwd_got.add((C.attn_fwd_loop(D, case.Sk, key[1], key[2]), D) + key + (T,))
            kerns = ("delta", "dkdv", "dq") if C.attn_bwd_two_kernel(case.Sk) else ("fused",)
            bwd_got |= {(kern,) + key + (case.dsum, T) for kern in kerns}
    print(f"forward instantiations {len(fwd_want)}, reached {len(fwd_want & fwd_got)}; backward kernel x flags "
          f"{len(bwd_want)}, reached {len(bwd_want & bwd_got)}; fp32 unit {len(f32_want)}, reached {len(f32_want & f32_got)}")
    assert {x[0] for x in fwd_want} == {"short", "double_buffered", "two_barrier"}
    assert fwd_want <= fwd_got, sorted(map(str, fwd_want - fwd_got))
    assert bwd_want <= bwd_got, sorted(map(str, bwd_want - bwd_got))
    assert f32_want <= f32_got, sorted(map(str, f32_want - f32_got))


# ----------------------------------------------------------------------------------------- exact cases
def _fwd_bwd(ops, T, p=0.0, seed=0, off=0):
    from apex.contrib.multihead_attn.attention import prepare_bias

    C = _C()
    B, H, Hk, Sq, Sk, D = ops.dims
    q, k, v, do = (t.to(DEV) for t in (ops.q, ops.k, ops.v, ops.do))
    bias = None if ops.bias is None else prepare_bias(ops.bias.to(DEV), B, H, Sq, Sk, T)
    kl = None if ops.k_lens is None else torch.tensor(ops.k_lens, dtype=torch.int32, device=DEV)
    o, lse, dmask = C.flash_attn_fwd(q, k, v, ops.causal, ops.scale, p, seed, off, kl, bias)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    C.flash_attn_bwd(do, q, k, v, o, lse, dq, dk, dv, ops.causal, ops.scale, p, seed, off, kl, dmask, None, 0, bias)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in (o, lse, dq, dk, dv))


def test_exact_shapes_reach_every_path():
    """The exact cases run on every forward loop (the bias cases cannot reach the short one, the uniform ones
    do) and on both backward schemes."""
    C = _C()
    uni = {(C.attn_fwd_loop(D, Sk, drop, False), C.attn_bwd_two_kernel(Sk)) for _, Sk, _, D in R.UNIFORM_SHAPES
           for drop in (False, True)}
    one = {(C.attn_fwd_loop(D, Sk, False, True), C.attn_bwd_two_kernel(Sk)) for _, Sk, D, _ in R.ONEHOT_SHAPES}
    print("uniform:", sorted(uni), "one-hot:", sorted(one))
    assert {x[0] for x in uni} == {"short", "two_barrier", "double_buffered"}
    assert {x[0] for x in one} == {"two_barrier", "double_buffered"}
    assert {x[1] for x in uni} == {x[1] for x in one} == {False, True}


def _exact_dtypes(D):
    return (BF16, F16, F32) if D <= 128 else (BF16, F16)


@pytest.mark.parametrize("shape", R.ONEHOT_SHAPES, ids=str)
def test_onehot_by_bias_is_bit_exact(shape):
    """q = 0 and a 0 / -inf bias: O[q] is V[pi(q)] bit for bit, lse = 0, dV[pi(q)] the dO rows that chose it,
    dK = dQ = 0 — every key <-> tile <-> lane mapping of the bias paths, forward and backward."""
    Sq, Sk, D, causal = shape
    for T in _exact_dtypes(D):
        ops, exp = R.onehot_operands(2, 3, Sq, Sk, D, T, causal)
        o, lse, dq, dk, dv = _fwd_bwd(ops, T)
        bad = {n: int((g.double() != e.double()).sum()) for n, g, e in
               (("O", o, exp["O"]), ("dV", dv, exp["dV"]), ("lse", lse, torch.zeros_like(lse)),
                ("dK", dk, torch.zeros_like(dk)), ("dQ", dq, torch.zeros_like(dq)))}
        print(f"onehot {shape} {R.DT_NAME[T]}: mismatching elements {bad}")
        assert not any(bad.values()), (shape, R.DT_NAME[T], bad)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "p0.5"])
@pytest.mark.parametrize("shape", R.UNIFORM_SHAPES, ids=str)
def test_uniform_counts_are_exact(shape, drop):
    """q = 0, no bias, n a power of two: n O and n dV are integer counts (of the kept keys with p = 0.5, whose
    rescale is exactly 2, from the NumPy mask) — the keep bit of every (query, key) on every path, forward and
    backward. dK = 0 exactly (q = 0). fp32: the forward is exact; the backward recomputes P from the rounded
    lse = log(n), so dV is within 2**-20 relative of the count (|lse| log2e rounded, one exp2 ulp, <= 16 E24)."""
    Sq, Sk, n, D = shape
    B, H, seed, off, thresh = 2, 3, 0xC0FFEE, 0x5EED, 128
    keep = torch.from_numpy(R.keep_mask(seed, off, B * H, Sq, Sk, thresh)).view(B, H, Sq, Sk) if drop else None
    for T in _exact_dtypes(D):
        ops, exp = R.uniform_operands(B, H, Sq, Sk, n, D, T, keep)
        o, lse, dq, dk, dv = _fwd_bwd(ops, T, 0.5 if drop else 0.0, seed, off)
        bad_o = int((o.double() != exp["O"].double()).sum())
        err_dv = float((dv.double() - exp["dV"].double()).abs().max())
        tol_dv = 0.0 if T != F32 else 2.0 ** -20 * float(exp["dV"].abs().max() + ops.do.double().abs().sum(1).max() / n)
        err_lse = float((lse.double() - exp["lse"]).abs().max())
        print(f"uniform {shape} drop={drop} {R.DT_NAME[T]}: O mismatches {bad_o}, max |dV - count / n| {err_dv:.3g} "
              f"(allowed {tol_dv:.3g}), |lse - log n| {err_lse:.3g}, max |dK| {float(dk.abs().max()):.3g}")
        assert bad_o == 0 and err_dv <= tol_dv, (shape, R.DT_NAME[T])
        assert err_lse <= 8 * R.E24 * exp["lse"] and float(dk.abs().max()) == 0.0
        assert bool(torch.isfinite(dq.float()).all())


# ----------------------------------------------------------------------------------------- guard bands
SENTINEL = 512.0


def _guarded(shape, dtype):
    """A [B, S, H, D] view inside a sentinel-filled buffer with gaps on the sequence and the head axis."""
    B, S, H, D = shape
    buf = torch.full((B, S + 4, H + 1, D), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:, 2:2 + S, :H]


def _guards_intact(buf, S, H):
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    inside[:, 2:2 + S, :H] = True
    return bool((buf[~inside] == SENTINEL).all())


@pytest.mark.parametrize("T", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("Sq,Sk,D,Hk", [(77, 100, 64, 3), (130, 193, 128, 3), (33, 65, 32, 1), (161, 129, 64, 1)])
def test_gradient_guard_bands(Sq, Sk, D, Hk, T):
    """dq / dk / dv as slices of wider sentinel-filled buffers (16-byte stores after lane swaps at ragged row
    counts; the group reduce with Hk < H): nothing outside the slices is written, and the values inside are the
    ones a plain call gives."""
    C = _C()
    B, H = 2, 3
    g = R._gen(f"guard-{Sq}-{Sk}-{D}")
    q, do = (torch.randn(B, Sq, H, D, generator=g).to(T).to(DEV) for _ in range(2))
    k, v = (torch.randn(B, Sk, Hk, D, generator=g).to(T).to(DEV) for _ in range(2))
    scale = 1.0 / math.sqrt(D)
    o, lse, dmask = C.flash_attn_fwd(q, k, v, True, scale, 0.0, 0, 0, None, None)
    plain = [torch.empty_like(t) for t in (q, k, v)]
    C.flash_attn_bwd(do, q, k, v, o, lse, *plain, True, scale, 0.0, 0, 0, None, dmask, None, 0, None)
    bufs, views = zip(*[_guarded(t.shape, T) for t in (q, k, v)])
    C.flash_attn_bwd(do, q, k, v, o, lse, *views, True, scale, 0.0, 0, 0, None, dmask, None, 0, None)
    torch.cuda.synchronize()
    ok = [_guards_intact(b, s, h) for b, s, h in zip(bufs, (Sq, Sk, Sk), (H, Hk, Hk))]
    same = [torch.equal(a, b) for a, b in zip(plain, views)]
    print(f"guards Sq {Sq} Sk {Sk} D {D} Hk {Hk} {R.DT_NAME[T]}: intact {ok}, equal to the plain call {same}")
    assert all(ok) and all(same)


@pytest.mark.parametrize("T", [BF16, F32], ids=["bf16", "f32"])
def test_grouped_packed_gradient_guard_bands(T):
    """The grouped packed layout [B, S, H + 2 Hk, D] as a slice of a wider sentinel buffer: dQ from the kernels and
    dK / dV from the group reduce land in their slices only; attention_grouped_packed on the same values gives
    the same gradient."""
    from apex.contrib.multihead_attn.attention import attention_grouped_packed

    C = _C()
    B, S, H, Hk, D = 2, 150, 2, 1, 64
    g = R._gen("guard-gpacked")
    qkv = torch.randn(B, S, H + 2 * Hk, D, generator=g).to(T).to(DEV)
    do = torch.randn(B, S, H, D, generator=g).to(T).to(DEV)
    q, k, v = qkv[:, :, :H], qkv[:, :, H:H + Hk], qkv[:, :, H + Hk:]
    scale = 1.0 / math.sqrt(D)
    o, lse, dmask = C.flash_attn_fwd(q, k, v, False, scale, 0.0, 0, 0, None, None)
    buf, view = _guarded((B, S, H + 2 * Hk, D), T)
    C.flash_attn_bwd(do, q, k, v, o, lse, view[:, :, :H], view[:, :, H:H + Hk], view[:, :, H + Hk:], False, scale, 0.0,
                     0, 0, None, dmask, None, 0, None)
    leaf = qkv.clone().requires_grad_(True)
    attention_grouped_packed(leaf, H, Hk).backward(do)
    torch.cuda.synchronize()
    ok, same = _guards_intact(buf, S, H + 2 * Hk), torch.equal(view, leaf.grad)
    print(f"grouped packed guards {R.DT_NAME[T]}: intact {ok}, equal to attention_grouped_packed's gradient {same}")
    assert ok and same


# ----------------------------------------------------------------------------------------- host side
def _small(T=BF16, B=2, Sq=40, Sk=72, H=2, D=64):
    g = R._gen("host")
    q, do = (torch.randn(B, Sq, H, D, generator=g).to(T).to(DEV) for _ in range(2))
    k, v = (torch.randn(B, Sk, H, D, generator=g).to(T).to(DEV) for _ in range(2))
    return q, k, v, do, 1.0 / math.sqrt(D)


def _bwd_args(q, k, v, do, scale, o, lse, over=()):
    a = dict(dout=do, q=q, k=k, v=v, o=o, lse=lse, dq=torch.empty_like(q), dk=torch.empty_like(k), dv=torch.empty_like(v),
             causal=False, scale=scale, p_drop=0.0, seed=0, offset=0, k_lens=None, dmask=None)
    a.update(dict(over))
    return a


def test_forward_refuses_operands_off_the_device():
    C = _C()
    q, k, v, do, scale = _small()
    kl_cpu = torch.tensor([72, 30], dtype=torch.int32)
    bias = torch.zeros(1, 1, 1, 72, dtype=BF16, device=DEV)
    bad = {"k on the CPU": dict(k=k.cpu()), "v on the CPU": dict(v=v.cpu()), "k_lens on the CPU": dict(k_lens=kl_cpu),
           "int64 k_lens": dict(k_lens=kl_cpu.long().to(DEV)), "bias on the CPU": dict(bias=bias.cpu()),
           "q on the CPU": dict(q=q.cpu(), k=k.cpu(), v=v.cpu())}
    for what, over in bad.items():
        a = dict(q=q, k=k, v=v, causal=False, scale=scale, p_drop=0.0, seed=0, offset=0, k_lens=None, bias=None)
        a.update(over)
        with pytest.raises(RuntimeError):
            C.flash_attn_fwd(**a)
        print("refused:", what)
    with pytest.raises(RuntimeError):
        C.flash_dropout_mask(1, 1, 4, 4, 0.1, 0, 0, torch.device("cpu"))


def test_backward_refuses_bad_operands():
    C = _C()
    q, k, v, do, scale = _small()
    o, lse, _ = C.flash_attn_fwd(q, k, v, False, scale, 0.0, 0, 0, None, None)
    _, _, dmask = C.flash_attn_fwd(q, k, v, False, scale, 0.5, 1, 2, None, None)
    bias = torch.zeros(1, 2, 1, 72, dtype=BF16, device=DEV)
    bad = {
        "o on the CPU": dict(o=o.cpu()), "dout on the CPU": dict(dout=do.cpu()), "lse on the CPU": dict(lse=lse.cpu()),
        "dq on the CPU": dict(dq=torch.empty_like(q).cpu()), "dk on the CPU": dict(dk=torch.empty_like(k).cpu()),
        "dv on the CPU": dict(dv=torch.empty_like(v).cpu()),
        "k_lens on the CPU": dict(k_lens=torch.tensor([72, 30], dtype=torch.int32)),
        "lse of another shape": dict(lse=lse[:, :, :-1].contiguous()), "lse transposed": dict(lse=lse.transpose(1, 2)),
        "lse not contiguous": dict(lse=torch.empty(2, 2, 80, device=DEV)[:, :, ::2]), "fp64 lse": dict(lse=lse.double()),
        "o of another dtype": dict(o=o.to(F16)), "o of another size": dict(o=o[:, :-8].contiguous()),
        "dout of another size": dict(dout=do[:, :-8].contiguous()), "dout of another dtype": dict(dout=do.float()),
        "dmask of another dtype": dict(p_drop=0.5, seed=1, offset=2, dmask=dmask.int()),
        "dmask on the CPU": dict(p_drop=0.5, seed=1, offset=2, dmask=dmask.cpu()),
        "dmask missing": dict(p_drop=0.5, seed=1, offset=2, dmask=None),
        "dbias on the CPU": dict(bias=bias, dbias=torch.zeros(1, 2, 1, 72)),
        "dsum on the CPU": dict(dsum=torch.zeros(2, 3, 2, 64)),
    }
    for what, over in bad.items():
        with pytest.raises(RuntimeError):
            C.flash_attn_bwd(**_bwd_args(q, k, v, do, scale, o, lse, over))
        print("refused:", what)
    C.flash_attn_bwd(**_bwd_args(q, k, v, do, scale, o, lse))      # the unmodified call is accepted
    # the bias-gradient column sums are a feature of the 16-bit units: refused for fp32 (found by a case)
    qf, kf, vf, dof = (t.float() for t in (q, k, v, do))
    of, lsef, _ = C.flash_attn_fwd(qf, kf, vf, False, scale, 0.0, 0, 0, None, None)
    with pytest.raises(RuntimeError):
        C.flash_attn_bwd(**_bwd_args(qf, kf, vf, dof, scale, of, lsef, dict(dsum=torch.zeros(2, 3, 2, 64, device=DEV))))
    print("refused: dsum with fp32 operands")
    torch.cuda.synchronize()


@pytest.mark.parametrize("T", [BF16, F32], ids=["bf16", "f32"])
def test_empty_shapes(T):
    """No key: O = 0, lse = +inf, zero gradients. No query: dK = dV = 0."""
    C = _C()
    for Sq, Sk in ((5, 0), (0, 7), (0, 0)):
        q, do = (torch.ones(2, Sq, 3, 64, dtype=T, device=DEV) for _ in range(2))
        k, v = (torch.ones(2, Sk, 3, 64, dtype=T, device=DEV) for _ in range(2))
        o, lse, dmask = C.flash_attn_fwd(q, k, v, False, 0.125, 0.0, 0, 0, None, None)
        dq, dk, dv = (torch.full_like(t, 7.0) for t in (q, k, v))
        C.flash_attn_bwd(do, q, k, v, o, lse, dq, dk, dv, False, 0.125, 0.0, 0, 0, None, dmask, None, 0, None)
        torch.cuda.synchronize()
        print(f"empty Sq {Sq} Sk {Sk} {R.DT_NAME[T]}: o {tuple(o.shape)} lse {tuple(lse.shape)}")
        assert o.shape == q.shape and lse.shape == (2, 3, Sq)
        assert bool((o == 0).all()) and bool((lse == R.INF).all())
        assert all(bool((t == 0).all()) for t in (dq, dk, dv))


@pytest.mark.parametrize("T", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("how", ["unaligned", "stride", "int64_k_lens", "cpu_k_lens", "packed_unaligned", "gpacked_stride"])
def test_wrapper_fallbacks_inside_bound(how, T):
    """Operands the binding refuses — a view off a 16-byte boundary, strides that are no multiple of 8 elements,
    int64 or CPU key lengths — still give a result through attention() / attention_packed() /
    attention_grouped_packed(), held to the same bound as every other case."""
    from apex.contrib.multihead_attn import attention as A

    B, S, H, D = 2, 77, 2, 64
    g = R._gen(f"fallback-{how}")
    q, k, v, do = (torch.randn(B, S, H, D, generator=g).to(T) for _ in range(4))
    k_lens = (77, 40) if "k_lens" in how else None
    Hk = 1 if how == "gpacked_stride" else H
    k, v = k[:, :, :Hk].contiguous(), v[:, :, :Hk].contiguous()
    ops = R.Ops(q, k, v, do, 1.0 / math.sqrt(D), True, k_lens)

    def odd(t, by):      # the same values in a view the binding refuses
        if by == "unaligned":
            flat = torch.zeros(t.numel() + 2, dtype=t.dtype, device=DEV)      # 4 or 8 bytes off
            return flat[2:].view(t.shape).copy_(t.to(DEV))
        wide = torch.zeros(*t.shape[:-1], t.shape[-1] + 4, dtype=t.dtype, device=DEV)
        return wide[..., :t.shape[-1]].copy_(t.to(DEV))

    if how in ("unaligned", "stride"):
        leaves = [odd(t, how).requires_grad_(True) for t in (q, k, v)]
        o = A.attention(*leaves, None, 0.0, True)
    elif how in ("int64_k_lens", "cpu_k_lens"):
        leaves = [t.to(DEV).requires_grad_(True) for t in (q, k, v)]
        kl = torch.tensor(k_lens, dtype=torch.int64, device=DEV if how == "int64_k_lens" else "cpu")
        o = A.attention(*leaves, None, 0.0, True, None, kl)
    elif how == "packed_unaligned":
        leaves = [odd(torch.stack([q, k, v], 2), "unaligned").requires_grad_(True)]
        o = A.attention_packed(leaves[0], None, 0.0, True)
    else:
        leaves = [odd(torch.cat([q, k, v], 2), "stride").requires_grad_(True)]
        o = A.attention_grouped_packed(leaves[0], H, Hk, None, 0.0, True)
    o.backward(do.to(DEV))
    torch.cuda.synchronize()
    if len(leaves) == 3:
        dq, dk, dv = (t.grad for t in leaves)
    elif how == "packed_unaligned":
        dq, dk, dv = leaves[0].grad.unbind(2)
    else:
        gr = leaves[0].grad
        dq, dk, dv = gr[:, :, :H], gr[:, :, H:H + Hk], gr[:, :, H + Hk:]
    got = {"O": R.bh(o.detach()).cpu(), "dQ": R.bh(dq).cpu(), "dK": R.bh(dk).cpu(), "dV": R.bh(dv).cpu()}
    ref = R.reference(ops, o.detach().cpu())
    fwd = "f32" if T == F32 else _C().attn_fwd_loop(D, S, False, False)
    _check_all(got, ref, R.bounds(ref, ops, T, stored="o"), f"fallback {how} {R.DT_NAME[T]}", fwd,
               "f32" if T == F32 else "fused", T)
