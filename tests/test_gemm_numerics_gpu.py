"""The MFMA GEMM kernels (csrc/gemm.hip) against the float64 reference of tests/gemm_reference.py: both
dtypes and every epilogue the launcher dispatches, on the one-tile-per-workgroup kernel (full and edge
tiles), the persistent kernel, the weight-gradient (transposed-read, split-K) form and C.transpose.

Two kinds of case per path. Exact cases: integer-valued operands whose every partial sum and result is
an integer of magnitude <= 256 and whose product has no two rows and no two columns alike
(tests/test_gemm_reference.py asserts both for every shape), expected values computed in int64 on the CPU
and compared with torch.equal — any mis-staged K-tile, swizzle slip, wrong buffer offset, misplaced fragment
or permuted tile shows as a wrong integer. Guard bands surround the outputs a caller provides (the
bias-gradient slot, the gemm_tt and gemm_tt_acc slots); C and the second [M, N] output are allocated by the
binding and cannot be guarded. Dense cases: seeded normal operands, held on every element to the bound derived in
gemm_reference.py (one rounding of the accumulator to T, the epilogue in fp32, one rounding of the
result), which tells erf from tanh GELU, one rounding from two, and a dropped bias from a kept one.
The binding's rejections (a foreign-device or misaligned bias, residual, stored activation or slot:
refused before anything is launched) and the wrappers' library fallbacks for the same operands are
checked too. Every test prints its figures before asserting; the worst error / bound per path,
epilogue, output and dtype is printed at the end.
"""
import pytest
import torch

import gemm_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F16, BF16 = R.F32, R.F16, R.BF16
DT_IDS = lambda t: R.DT_NAME[t]  # noqa: E731
GUARD = -768.0   # (exact in bf16 and fp16)
CASES = {"n": 0}


def _C():
    import apex

    return apex._ext.require()


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    R.WORST.clear()
    CASES["n"] = 0
    yield
    _C().set_gemm_persist(0, -1)


@pytest.fixture(autouse=True)
def _persist_choice():
    yield
    _C().set_gemm_persist(0, -1)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _gemm(epi, A, B, bias=None, aux=None, bdt=None, slot=None):
    C = _C()
    return C.gemm(A, B, getattr(C, R.epi_attr(epi)), bias if R.has_bias(epi) else None, aux if R.aux_in(epi) else None,
                  bdt if R.colsum(epi) else None, slot)


def _offset16(t):
    """t's values in a tensor that starts 16 bytes into its storage."""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    flat[8:] = t.reshape(-1).to(DEV)
    v = flat[8:].view(t.shape)
    assert v.data_ptr() % 16 == 0 and v.storage_offset() == 8
    return v


def _column_slice(t):
    """t's values as a column slice of a wider matrix (leading dimension K + 128)."""
    wide = torch.full((t.shape[0], t.shape[1] + 128), 3.0, dtype=t.dtype, device=DEV)
    wide[:, 64:64 + t.shape[1]] = t.to(DEV)
    v = wide[:, 64:64 + t.shape[1]]
    assert v.stride(0) == t.shape[1] + 128 and not v.is_contiguous()
    return v


def _device_operands(shape, A, B):
    Ad, Bd = A.to(DEV), B.to(DEV)
    if shape.layout == "lda":
        Ad = _column_slice(A)
    elif shape.layout == "ldb":
        Bd = _column_slice(B)
    elif shape.layout == "a3d":
        Ad = Ad.view(2, shape.M // 2, shape.K)
    elif shape.layout == "offset16":
        Ad, Bd = _offset16(A), _offset16(B)
    return Ad, Bd


def _dense(shape, T, persist, on_device=False):
    """Every epilogue of one shape and dtype against the bound. on_device: the float64 reference (a torch
    float64 product, independent of the kernel under test) and the comparison run on the GPU."""
    C = _C()
    C.set_gemm_persist(0, 1 if persist else 0)
    A, B, bias, aux = R.dense_operands(shape.name, shape.M, shape.N, shape.K, T)
    Ad, Bd = _device_operands(shape, A, B)
    bd, xd = bias.to(DEV), aux.to(DEV)
    if shape.layout == "a3d":
        xd = xd.view(2, shape.M // 2, shape.N)  # (aux is checked by shape: C's shape is accepted)
    if on_device:
        acc, cond = R.acc_ref(A.to(DEV), B.to(DEV))
        bias, aux = bd, aux.to(DEV)
    else:
        acc, cond = R.acc_ref(A, B)
    for epi in shape.epis:
        for bdt in ((F32, T) if R.colsum(epi) else (None,)):
            c, x = _gemm(epi, Ad, Bd, bd, xd, bdt)
            assert c.shape[:-1] == Ad.shape[:-1] and c.shape[-1] == shape.N
            r = R.check_epilogue(epi, T, shape.K, acc, cond, c, x, bias, aux, bdt,
                                 what=f"{shape.name} {R.DT_NAME[T]}", tag=shape.path)
            CASES["n"] += 1
            print(f"{shape.name} {R.DT_NAME[T]} {epi} db={R.DT_NAME[bdt]}: worst error / bound {r:.3f}")


def _exact(shape, T, persist):
    """The integer cases: bit-exact C for NONE / BIAS / RESID / MUL, H of BIAS_GELU, the fp32 bias gradient of
    MUL written into a slot of a guarded buffer (at an odd element offset: partial_colsum stores scalars)."""
    C = _C()
    C.set_gemm_persist(0, 1 if persist else 0)
    A, B, bias, aux = R.exact_operands(shape.M, shape.N, shape.K)
    Ad, Bd = _device_operands(shape, A.to(T), B.to(T))
    bd, xd = bias.to(T).to(DEV), aux.to(T).to(DEV)
    for epi in (e for e in R.EXACT_EPIS if e in shape.epis):
        exp = R.exact_expected(epi, A, B, bias, aux)
        guard = torch.full((shape.N + 64,), GUARD, device=DEV)
        slot = guard[17:17 + shape.N] if epi == "mul" else None
        c, x = _gemm(epi, Ad, Bd, bd, xd, F32, slot)
        CASES["n"] += 1
        for name, want in exp.items():
            got = (c if name == "C" else x).reshape(want.shape).cpu()
            bad = int((got.double() != want.double()).sum())
            print(f"{shape.name} {R.DT_NAME[T]} exact {epi} {name}: {bad} of {want.numel()} elements differ")
            assert torch.equal(got.double(), want.double()), (shape.name, epi, name)
        if epi == "mul":
            assert x.data_ptr() == slot.data_ptr() and x.dtype == F32
            g = guard.cpu()
            assert bool((g[:17] == GUARD).all()) and bool((g[17 + shape.N:] == GUARD).all()), "guard band written"


# ----------------------------------------------------------------------------
# one tile per workgroup: full tiles, edge tiles, operand layouts
# ----------------------------------------------------------------------------
ONE_TILE = R.FULL + R.EDGE + R.LAYOUT


@pytest.mark.parametrize("T", R.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", ONE_TILE, ids=[s.name for s in ONE_TILE])
def test_one_tile_dense(shape, T):
    _dense(shape, T, persist=False)


@pytest.mark.parametrize("T", R.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", ONE_TILE, ids=[s.name for s in ONE_TILE])
def test_one_tile_exact(shape, T):
    _exact(shape, T, persist=False)


# ----------------------------------------------------------------------------
# persistent kernel: shapes from the CU count
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("T", R.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("which", range(4), ids=["two-tiles-k64", "two-tiles-k128", "two-tiles-k192", "three-tiles"])
def test_persistent_dense(which, T):
    cus = _cus()
    shape = R.persist_shapes(cus)[which]
    tiles = (shape.M // 256) * (shape.N // 256)
    print(f"{cus} CUs, {tiles} tiles, grid {(cus // 8) * 8}")
    assert tiles > cus and shape.M % 256 == 0 and shape.N % 256 == 0
    assert which < 3 or tiles > 2 * ((cus // 8) * 8)
    _dense(shape, T, persist=True, on_device=True)


@pytest.mark.parametrize("T", R.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("which", [1, 3], ids=["two-tiles-k128", "three-tiles"])
def test_persistent_exact(which, T):
    shape = R.persist_shapes(_cus())[which]
    assert (shape.M // 256) * (shape.N // 256) > _cus()
    _exact(shape, T, persist=True)


def test_persistent_matches_one_tile_bitwise():
    """Same operands through both kernels: the outputs are the same bits (the case the persistent file pins at
    K = 1024, here at one and three K-tiles with an epilogue that reads and one that writes a second output)."""
    C = _C()
    shape = R.persist_shapes(_cus())[0]
    for K, T in ((64, F16), (192, BF16)):
        A, B, bias, aux = (t.to(DEV) for t in R.dense_operands(f"pvo-{K}", shape.M, shape.N, K, T))
        for epi in ("bias_gelu_d", "mul"):
            C.set_gemm_persist(0, 0)
            c0, x0 = _gemm(epi, A, B, bias, aux, F32)
            C.set_gemm_persist(0, 1)
            c1, x1 = _gemm(epi, A, B, bias, aux, F32)
            assert torch.equal(c0, c1) and torch.equal(x0, x1), (K, epi)


# ----------------------------------------------------------------------------
# weight-gradient form
# ----------------------------------------------------------------------------
def _slot(P, Q, dtype, fill=GUARD):
    """A [P, Q] slot 16 bytes into a larger guarded buffer."""
    off = 16 // torch.empty((), dtype=dtype).element_size()
    guard = torch.full((P * Q + 2 * off + 64,), fill, dtype=dtype, device=DEV)
    return guard, guard[off:off + P * Q].view(P, Q), off


def _guard_ok(guard, off, n):
    g = guard.cpu().float()
    return bool((g[:off] == GUARD).all()) and bool((g[off + n:] == GUARD).all())


@pytest.mark.parametrize("T", R.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", R.WGRAD, ids=[f"r{r}-{p}x{q}-s{s}" for (r, p, q, s) in R.WGRAD])
def test_wgrad_dense(case, T):
    C = _C()
    Rr, P, Q, s = case
    A, B = R.dense_wgrad_operands(f"{Rr}x{P}x{Q}", Rr, P, Q, T)
    Ad, Bd = A.to(DEV), B.to(DEV)
    assert C.gemm_tt_supported(Ad, Bd, s)
    runs = [(F32, False), (T, False), (F32, True), (T, True)]   # (output dtype, out= a slot view)
    for odt, slotted in runs:
        ref, bound = R.wgrad_expected(A, B, s, odt)
        guard, slot, off = _slot(P, Q, odt) if slotted else (None, None, 0)
        out = C.gemm_tt(Ad, Bd, s, odt, out=slot)
        assert out.dtype == odt and out.shape == (P, Q)
        # (one slice, T, no slot: the kernel's own T epilogue; everything else goes through fp32 slabs)
        kind = "direct" if (s == 1 and odt == T and not slotted) else ("one slab" if s == 1 else "slabs")
        r = R.check(out, ref, bound, f"wgrad r{Rr} {P}x{Q} s{s} -> {R.DT_NAME[odt]}",
                    f"wgrad {kind} {R.DT_NAME[T]}->{R.DT_NAME[odt]}")
        CASES["n"] += 1
        print(f"wgrad r{Rr} {P}x{Q} s{s} {R.DT_NAME[T]} -> {R.DT_NAME[odt]} slot={slotted}: worst error / bound {r:.3f}")
        if slotted:
            assert out.data_ptr() == slot.data_ptr() and _guard_ok(guard, off, P * Q), "guard band written"


@pytest.mark.parametrize("T", R.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("pq", R.WGRAD_PQ, ids=[f"{p}x{q}" for (p, q) in R.WGRAD_PQ])
def test_wgrad_exact(pq, T):
    C = _C()
    P, Q = pq
    for Rr, splits in ((192, (1, 3)), (448, (5,))):
        A, B, _, _ = R.exact_operands(P, Q, Rr)
        want = R.exact_acc(A, B).double()
        Ad, Bd = A.t().contiguous().to(T).to(DEV), B.t().contiguous().to(T).to(DEV)
        for s in splits:
            for odt in (T, F32):
                guard, slot, off = _slot(P, Q, odt)
                outs = [C.gemm_tt(Ad, Bd, s, odt), C.gemm_tt(Ad, Bd, s, odt, out=slot)]
                CASES["n"] += 2
                for out in outs:
                    assert torch.equal(out.cpu().double(), want), (P, Q, Rr, s, odt)
                assert _guard_ok(guard, off, P * Q), "guard band written"
        # accumulation into an fp32 buffer with integer previous contents, inside guard bands
        guard, slot, off = _slot(P, Q, F32)
        prev = ((torch.arange(P)[:, None] * 3 + torch.arange(Q)[None, :]) % 11 - 5).double()
        slot.copy_(prev.to(DEV))
        C.gemm_tt_acc(Ad, Bd, slot)
        CASES["n"] += 1
        assert torch.equal(slot.cpu().double(), prev + want) and _guard_ok(guard, off, P * Q)


@pytest.mark.parametrize("T", R.DTYPES, ids=DT_IDS)
def test_wgrad_acc_dense(T):
    """gemm_tt_acc on partial-tile shapes with nonzero previous contents."""
    C = _C()
    for (Rr, P, Q) in ((192, 200, 264), (320, 8, 1608), (64, 520, 256)):
        A, B = R.dense_wgrad_operands(f"{Rr}x{P}x{Q}", Rr, P, Q, T)
        prev = torch.randn(P, Q, generator=R._gen("prev"))
        out = prev.to(DEV).clone()
        C.gemm_tt_acc(A.to(DEV), B.to(DEV), out)
        ref, bound = R.wgrad_expected(A, B, 1, F32, prev)
        r = R.check(out, ref, bound, f"wgrad_acc r{Rr} {P}x{Q}", f"wgrad acc {R.DT_NAME[T]}->f32")
        CASES["n"] += 1
        print(f"wgrad_acc r{Rr} {P}x{Q} {R.DT_NAME[T]}: worst error / bound {r:.3f}")


# ----------------------------------------------------------------------------
# C.transpose
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("T", R.DTYPES, ids=DT_IDS)
def test_transpose_bit_exact(T):
    C = _C()
    for (r, c) in R.TRANSPOSE_SHAPES:
        x = torch.randn(r, c, generator=R._gen(f"tr{r}x{c}")).to(T).to(DEV)
        assert torch.equal(C.transpose(x), x.t().contiguous()), (r, c)
        wide = torch.randn(r, c + 5, generator=R._gen(f"trw{r}x{c}")).to(T).to(DEV)
        v = wide[:, 3:3 + c]                       # non-contiguous
        assert not v.is_contiguous() or r == 1
        assert torch.equal(C.transpose(v), v.t().contiguous()), (r, c, "non-contiguous")
        flat = torch.randn(r * c + 8, generator=R._gen(f"trm{r}x{c}")).to(T).to(DEV)
        m = flat[1:1 + r * c].view(r, c)           # contiguous, data pointer 2 bytes off 16-byte alignment
        assert m.data_ptr() % 16 != 0
        assert torch.equal(C.transpose(m), m.t().contiguous()), (r, c, "misaligned")
        CASES["n"] += 3
    with pytest.raises(RuntimeError):
        C.transpose(torch.zeros(8, 8, device=DEV))  # fp32
    with pytest.raises(RuntimeError):
        C.transpose(torch.zeros(8, 8, dtype=T))     # not on the device


# ----------------------------------------------------------------------------
# what the binding refuses, and what the wrappers do then
# ----------------------------------------------------------------------------
def _misaligned(t):
    """t's values, contiguous, at a data pointer one element past 16-byte alignment."""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    flat[1:1 + t.numel()] = t.reshape(-1).to(DEV)
    v = flat[1:1 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


@pytest.mark.parametrize("T", R.DTYPES, ids=DT_IDS)
def test_binding_rejections(T):
    """Operands the kernels cannot read are refused by the binding's checks, which all precede the launch."""
    C = _C()
    M, N, K = 256, 264, 128
    A, B, bias, aux = R.dense_operands("reject", M, N, K, T)
    Ad, Bd, bd, xd = A.to(DEV), B.to(DEV), bias.to(DEV), aux.to(DEV)
    assert C.gemm_supported(Ad, Bd)
    assert not C.gemm_supported(Ad, B) and not C.gemm_supported(A, Bd)
    assert not C.gemm_supported(Ad, _misaligned(B)) and not C.gemm_supported(_misaligned(A), Bd)

    def refused(*args):
        with pytest.raises(RuntimeError):
            C.gemm(*args)

    refused(Ad, B, C.EPI_NONE)
    refused(Ad, Bd, C.EPI_BIAS, bias)                               # CPU bias
    refused(Ad, Bd, C.EPI_BIAS_GELU, _misaligned(bias))             # a view one element into a buffer
    refused(Ad, Bd, C.EPI_BIAS_GELU_D, bd[:N - 8])                  # not N elements
    refused(Ad, Bd, C.EPI_BIAS, torch.cat([bd, bd])[::2])           # not contiguous
    refused(Ad, Bd, C.EPI_RESID, None, aux)                         # CPU residual
    refused(Ad, Bd, C.EPI_RESID, None, _misaligned(aux))
    refused(Ad, Bd, C.EPI_MUL, None, _misaligned(aux), F32)
    refused(Ad, Bd, C.EPI_DGELU, None, xd.view(N, M), F32)          # numel fits, the shape does not
    refused(Ad, Bd, C.EPI_MUL, None, xd.view(-1), F32)
    refused(Ad, Bd, C.EPI_MUL, None, xd, F32, torch.zeros(N))       # CPU slot
    refused(Ad, Bd, C.EPI_MUL, None, xd, F32, torch.zeros(N, dtype=T, device=DEV))   # slot of another dtype
    refused(Ad, Bd, C.EPI_MUL, None, xd, F32, torch.zeros(N + 8, device=DEV))
    # accepted: C-shaped aux, and a bias-gradient slot at any element offset
    c, db = C.gemm(Ad, Bd, C.EPI_MUL, None, xd, F32, torch.zeros(N + 8, device=DEV)[3:3 + N])
    assert db.data_ptr() % 16 != 0

    a, b = torch.randn(128, 256, device=DEV).to(T), torch.randn(128, 264, device=DEV).to(T)
    assert C.gemm_tt_supported(a, b, 2)
    assert not C.gemm_tt_supported(a, b.cpu(), 2) and not C.gemm_tt_supported(a, _misaligned(b), 2)
    with pytest.raises(RuntimeError):
        C.gemm_tt(a, b.cpu(), 2, F32)
    with pytest.raises(RuntimeError):
        C.gemm_tt(a, b, 2, F32, out=_misaligned(torch.zeros(256, 264)))
    with pytest.raises(RuntimeError):
        C.gemm_tt(a, b, 2, F32, out=torch.zeros(256, 264))
    with pytest.raises(RuntimeError):
        C.gemm_tt(a, b, 1, T, out=torch.zeros(256, 264, device=DEV))    # dtype
    with pytest.raises(RuntimeError):
        C.gemm_tt_acc(a, b, torch.zeros(256, 264))
    with pytest.raises(RuntimeError):
        C.gemm_tt_acc(a, b, _misaligned(torch.zeros(256, 264)))
    with pytest.raises(RuntimeError):
        C.gemm_tt_acc(a, b.cpu(), torch.zeros(256, 264, device=DEV))


@pytest.mark.parametrize("T", R.DTYPES, ids=DT_IDS)
def test_wrapper_fallbacks(T, monkeypatch):
    """apex.ops.gemm with operands the binding refuses: each wrapper takes its library path and still computes
    the same function. The library composition rounds the product to T and then applies the epilogue in
    fp32, which is what the BIAS_GELU_D / MUL / DGELU / RESID bounds describe."""
    from apex.ops import gemm as G

    monkeypatch.setattr(G, "_MODE", "mfma")   # every supported product on the MFMA kernels: what falls back below
    M, N, K = 300, 264, 128                   # does so because of its operand alone
    A, B, bias, aux = R.dense_operands("fallback", M, N, K, T)
    Ad, Bd, bd = A.to(DEV), B.to(DEV), bias.to(DEV)
    acc, cond = R.acc_ref(A, B)
    tag = "fallback"

    for bad_bias in (_misaligned(bias), bias):                      # a misaligned view; a CPU tensor
        y = G.linear(Ad, Bd, bad_bias)
        R.check(y, *R.expected("bias", T, K, acc, cond, bias)["C"], "linear fallback", f"{tag} bias C {R.DT_NAME[T]}")
        y, h = G.linear_gelu(Ad, Bd, bad_bias)
        exp = R.expected("bias_gelu_d", T, K, acc, cond, bias)
        R.check(y, *exp["C"], "linear_gelu fallback Y", f"{tag} bias_gelu C {R.DT_NAME[T]}")
        R.check(h, *R.expected("bias", T, K, acc, cond, bias)["C"], "linear_gelu fallback H", f"{tag} bias_gelu X {R.DT_NAME[T]}")
        y, g = G.linear_gelu_d(Ad, Bd, bad_bias, act=G.ACT_GELU_TANH)
        exp = R.expected("bias_gelu_tanh_d", T, K, acc, cond, bias)
        R.check(y, *exp["C"], "linear_gelu_d fallback Y", f"{tag} bias_gelu_tanh_d C {R.DT_NAME[T]}")
        R.check(g, *exp["X"], "linear_gelu_d fallback G", f"{tag} bias_gelu_tanh_d X {R.DT_NAME[T]}")
    # the aligned call takes the kernel and passes the kernel's own check
    y, h = G.linear_gelu(Ad, Bd, bd)
    R.check_epilogue("bias_gelu", T, K, acc, cond, y, h, bias, what="linear_gelu")

    # input-gradient wrappers: dy [M, K] @ w [K, N] -> [M, N], i.e. A = dy, B = w^T
    w = Bd.t().contiguous()
    for bad in (_misaligned(aux), aux):
        out = G.dgrad_resid(Ad, w, bad)
        R.check(out, *R.expected("resid", T, K, acc, cond, aux=aux)["C"], "dgrad_resid fallback", f"{tag} resid C {R.DT_NAME[T]}")
        dh, db = G.dgrad_mul(Ad, w, bad, F32)
        R.check_epilogue("mul", T, K, acc, cond, dh, db, aux=aux, bdt=F32, what="dgrad_mul fallback", tag=tag)
        dh, db = G.dgrad_dgelu(Ad, w, bad, T)
        R.check_epilogue("dgelu", T, K, acc, cond, dh, db, aux=aux, bdt=T, what="dgrad_dgelu fallback", tag=tag)
    # a slot the binding would refuse (another dtype): the library path, which returns its own tensor
    dh, db = G.dgrad_mul(Ad, w, aux.to(DEV), F32, bias_grad_out=torch.zeros(N, dtype=T, device=DEV))
    R.check_epilogue("mul", T, K, acc, cond, dh, db, aux=aux, bdt=F32, what="dgrad_mul slot fallback", tag=tag)



def _misaligned_slot(P, Q, dtype):
    """A contiguous [P, Q] slot one element into a guarded buffer (not 16-byte aligned)."""
    guard = torch.full((P * Q + 9,), GUARD, dtype=dtype, device=DEV)
    slot = guard[1:1 + P * Q].view(P, Q)
    assert slot.data_ptr() % 16 != 0
    return guard, slot


@pytest.mark.parametrize("T", R.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", ["auto", "mfma"])
@pytest.mark.parametrize("tokens", [256, 8192], ids=["one-slice", "split-k"])
def test_wgrad_misaligned_slot(tokens, mode, T, monkeypatch):
    """fused._wgrad with a slot the split-K reduction's 16-byte stores cannot take, without and with split-K
    (8192 tokens: eight slices), on the library path (auto: bmm slabs + splitk_reduce) and on gemm_tt (mfma):
    the kernels never see the slot, which is filled by a copy; and accumulate_main_grad with such a main_grad."""
    from apex.ops import fused
    from apex.ops import gemm as G

    C = _C()
    monkeypatch.setattr(G, "_MODE", mode)
    P, Q = 256, 264
    s = fused._wgrad_splits(tokens, P, Q)
    assert (s > 1) == (tokens == 8192)
    a, b = R.dense_wgrad_operands(f"slot-{tokens}", tokens, P, Q, T)
    ad, bd = a.to(DEV), b.to(DEV)
    guard, slot = _misaligned_slot(P, Q, T)
    out = fused._wgrad(ad, bd, out=slot)
    ref, bound = R.wgrad_expected(a, b, s, T)
    r = R.check(out, ref, bound, f"_wgrad misaligned slot {tokens} {mode}", f"fallback wgrad {mode} {R.DT_NAME[T]}")
    print(f"_wgrad {tokens} tokens, {s} slices, {mode}: worst error / bound {r:.3f}")
    g = guard.cpu().float()
    assert out.data_ptr() == slot.data_ptr() and g[0] == GUARD and bool((g[1 + P * Q:] == GUARD).all())
    # the binding refuses the slot outright
    slabs = torch.zeros(2, P, Q, device=DEV)
    with pytest.raises(RuntimeError):
        C.splitk_reduce(slabs, T, slot)
    with pytest.raises(RuntimeError):
        C.splitk_reduce(slabs, T, torch.zeros(P, Q, dtype=T))
    # fp32 main_grad accumulation into a misaligned buffer
    guard, mg = _misaligned_slot(P, Q, F32)
    prev = torch.randn(P, Q, generator=R._gen("prev"))
    mg.copy_(prev.to(DEV))
    fused.accumulate_main_grad(mg, ad, bd)
    ref, bound = R.wgrad_expected(a, b, s, F32, prev)
    R.check(mg, ref, bound, f"main_grad misaligned {tokens} {mode}", f"fallback main_grad {mode} {R.DT_NAME[T]}")
    g = guard.cpu()
    assert g[0] == GUARD and bool((g[1 + P * Q:] == GUARD).all())


def test_fp8_wgrad_misaligned_slot():
    """Fp8State.wgrad shares splitk_reduce: an unaligned slot receives a copy of the same bits."""
    from apex import fp8

    C = _C()
    st = fp8.Fp8State(device=DEV)
    assert st.wgrad_enabled()
    Rr, P, Q = 1024, 256, 272
    one = torch.ones(1, device=DEV)
    g = R._gen("fp8-slot")
    d = (C.fp8_quantize(torch.randn(Rr, P, generator=g).bfloat16().to(DEV), st._bwd, one), one)
    x = (C.fp8_quantize(torch.randn(Rr, Q, generator=g).bfloat16().to(DEV), st._fwd, one), one)
    want = st.wgrad(d, x, BF16)
    assert want is not None and want.shape == (P, Q)
    guard, slot = _misaligned_slot(P, Q, BF16)
    got = st.wgrad(d, x, BF16, out=slot)
    gd = guard.cpu().float()
    assert got.data_ptr() == slot.data_ptr() and torch.equal(got, want)
    assert gd[0] == GUARD and bool((gd[1 + P * Q:] == GUARD).all())


def test_zz_summary():
    """Prints the worst error / bound per path, epilogue, output and dtype seen by this file's tests."""
    print(f"\n{CASES['n']} kernel cases checked; worst |got - ref| / bound per path, epilogue, output and dtype:")
    for tag in sorted(R.WORST):
        print(f"  {tag}: {R.WORST[tag][0]:.3f}  ({R.WORST[tag][1]})")
    assert all(v[0] <= 1.0 for v in R.WORST.values())
