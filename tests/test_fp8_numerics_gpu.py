"""The fp8 kernels (csrc/fp8.hip, csrc/fp8_pack.h, the uint8 instantiations of the MFMA GEMM, gemm_tt_f8, the Q8
side outputs of the GEMM epilogue) against tests/fp8_reference.py.

Quantisers, amax and update_scales are compared to the bit with a codec written from the OCP specification
(tests/test_fp8_reference.py anchors it to torch's CPU casts): every finite bf16 / fp16 pattern and an fp32
boundary set at five scales, every length class and tile shape, current and delayed scaling, non-finite
elements. The GEMMs: integer-coded operands bit-exact, dense operands across the whole code range held on
every element of every output to the bound derived in fp8_reference.py, the persistent kernel bit-identical
to the one-tile kernel, the Q8 codes and amax exact given the stored C. The bindings' refusals are asserted for
every operand. Every test prints its figures before asserting; the worst error / bound per kernel, output,
format and dtype is printed at the end and written to the file named by FP8_NUMERICS_WORST_OUT.
"""
import os

import pytest
import torch

import fp8_reference as F
import gemm_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F16, BF16 = F.F32, F.F16, F.BF16
DT_IDS = lambda t: F.DT_NAME[t]  # noqa: E731
FMT_IDS = lambda f: F.FMT_NAME[f]  # noqa: E731
GUARD = -768.0
CASES = {"n": 0}
EXACT = {}     # tag -> elements that differed in the bit-exact comparisons (0 everywhere for a pass)
ACC_MEAS = {}  # kernel form -> worst |err| / (2**-24 cond) of the dense cases (the measurement behind F.ACC_HW)
NOTES = []


def _acc_measure(form, got, ref, cond, rounding=0.0, tiny=0.0):
    """Worst accumulator error in units of 2**-24 cond: |err| less what the roundings after the accumulator can
    account for (a 16-bit C: (u + 2**-24) |ref| + tiny), so a lower estimate there and the error itself in fp32."""
    err = (got.detach().to(ref.device).double() - ref).abs() - rounding * ref.abs() - tiny
    r = float((err.clamp(min=0.0) / (F.E24 * cond)).max())
    ACC_MEAS[form] = max(ACC_MEAS.get(form, 0.0), r)
    return r


def _C():
    import apex

    return apex._ext.require()


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    R.WORST.clear()
    EXACT.clear()
    ACC_MEAS.clear()
    del NOTES[:]
    CASES["n"] = 0
    yield
    _C().set_gemm_persist(1, -1)


@pytest.fixture(autouse=True)
def _persist_choice():
    yield
    _C().set_gemm_persist(1, -1)


def _scalar(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


def _same(got, want, tag, what=""):
    """Bit-exact comparison of every element (NaN equal to NaN); the count of differing elements goes under tag."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.is_floating_point:
        bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    else:
        bad = got != want
    n = int(bad.sum())
    EXACT[tag] = EXACT.get(tag, 0) + n
    CASES["n"] += 1
    if n:
        i = bad.reshape(-1).nonzero()[:4].reshape(-1).tolist()
        raise AssertionError(f"{tag} {what}: {n} of {want.numel()} elements differ, first at {i}: got "
                             f"{got.reshape(-1)[i].tolist()}, want {want.reshape(-1)[i].tolist()}")


def _val(t, want, tag, what=""):
    """One fp32 device value against a Python float, to the bit."""
    _same(t.reshape(-1)[:1].float(), torch.tensor([want], dtype=torch.float32), tag, what)


# ----------------------------------------------------------------------------
# fp8_quantize
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", F.FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("dt", F.IN_DTYPES, ids=DT_IDS)
def test_quantize_tables(dt, fmt):
    """All finite 16-bit patterns (fp32: the boundary set) at five scales and three length classes: codes and amax."""
    C = _C()
    table = F.quant_table(dt, fmt)
    L = table.numel()
    table_d = table.to(DEV)
    tag = f"quantize {F.FMT_NAME[fmt]} {F.DT_NAME[dt]}"
    idx = {n: F.table_index(n, L) for n in F.QUANT_LENGTHS}
    want_amax = {n: F.amax_ref(table[idx[n]]) for n in F.QUANT_LENGTHS}
    assert len(torch.unique(idx[F.QUANT_LENGTHS[2]])) == L           # the long case holds every table entry
    for s in F.SCALES:
        ref_d = F.quantize_ref(table, s, fmt).to(DEV)
        for n in F.QUANT_LENGTHS:
            i_d = idx[n].to(DEV)
            x = table_d[i_d].contiguous()
            amax = torch.zeros(1, device=DEV)
            y = C.fp8_quantize(x, fmt, _scalar(s), amax)
            assert y.dtype == torch.uint8 and y.shape == x.shape
            bad = int((y != ref_d[i_d]).sum())
            print(f"{tag} s={s:g} n={n}: {bad} codes differ, amax {float(amax):g}")
            _same(y, ref_d[i_d], tag + " codes", f"s={s:g} n={n}")
            _val(amax, want_amax[n], tag + " amax", f"s={s:g} n={n}")
    # a larger pre-filled amax stays; amax = None works; an empty input launches nothing
    x = table_d[idx[F.QUANT_LENGTHS[1]].to(DEV)].contiguous()
    big = 3.4e38
    assert big > F.amax_ref(table)
    amax = _scalar(big)
    y = C.fp8_quantize(x, fmt, _scalar(37.5), amax)
    _val(amax, F.f32(big), tag + " amax", "pre-filled")
    _same(C.fp8_quantize(x, fmt, _scalar(37.5)), y, tag + " codes", "amax=None")
    e = C.fp8_quantize(x[:0], fmt, _scalar(37.5), amax)
    assert e.shape == (0,) and e.dtype == torch.uint8


@pytest.mark.parametrize("fmt", F.FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("dt", F.IN_DTYPES, ids=DT_IDS)
def test_quantize_current_scaling(dt, fmt):
    """cur_amax given: scale = fl32(smax / a) and scale_inv = fl32(1 / scale) are written, the codes use that
    scale; a = 0, inf, NaN give scale 1."""
    C = _C()
    g = R._gen(f"cur-{F.DT_NAME[dt]}")
    x = (torch.randn(8 * 256 + 5, generator=g) * 3).to(dt)
    xd = x.to(DEV)
    tag = f"quantize current {F.FMT_NAME[fmt]} {F.DT_NAME[dt]}"
    for smax in (F.FMT_MAX[fmt], F.FMT_MAX[fmt] * 0.5):
        for a in (F.amax_ref(x), 0.37, 448.0, 1e-30, 3e38, 0.0, float("inf"), float("nan")):
            s_ref, sinv_ref = F.current_scale(a, smax)
            scale, sinv = torch.full((1,), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
            y = C.fp8_quantize(xd, fmt, scale, None, _scalar(a), sinv, smax)
            print(f"{tag} smax={smax:g} a={a:g}: scale {float(scale)!r} (ref {s_ref!r}), scale_inv {float(sinv)!r} (ref {sinv_ref!r})")
            _val(scale, s_ref, tag + " scale", f"a={a:g}")
            _val(sinv, sinv_ref, tag + " scale_inv", f"a={a:g}")
            _same(y, F.quantize_ref(x, s_ref, fmt), tag + " codes", f"a={a:g}")
            if a in (0.0, float("inf")) or a != a:
                assert s_ref == 1.0 and sinv_ref == 1.0


# ----------------------------------------------------------------------------
# fp8_quantize_t
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", F.FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("dt", F.IN_DTYPES, ids=DT_IDS)
def test_quantize_t(dt, fmt):
    C = _C()
    table = F.quant_table(dt, fmt)
    tag = f"quantize_t {F.FMT_NAME[fmt]} {F.DT_NAME[dt]}"
    for (r, c) in F.QT_SHAPES:
        # delayed scaling on table values
        x = table[F.table_index(r * c, table.numel())].view(r, c).contiguous()
        amax = torch.zeros(1, device=DEV)
        yt = C.fp8_quantize_t(x.to(DEV), fmt, _scalar(37.5), amax)
        assert yt.shape == (c, r)
        _same(yt, F.quantize_ref(x, 37.5, fmt).t().contiguous(), tag + " codes", f"{r}x{c} delayed")
        _val(amax, F.amax_ref(x), tag + " amax", f"{r}x{c}")
        # current scaling on normal values
        x = (torch.randn(r, c, generator=R._gen(f"qt-{r}x{c}")) * 3).to(dt)
        a = F.amax_ref(x)
        smax = F.FMT_MAX[fmt] * 0.5
        s_ref, sinv_ref = F.current_scale(a, smax)
        scale, sinv = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        yt = C.fp8_quantize_t(x.to(DEV), fmt, scale, None, _scalar(a), sinv, smax)
        _val(scale, s_ref, tag + " scale", f"{r}x{c}")
        _val(sinv, sinv_ref, tag + " scale_inv", f"{r}x{c}")
        _same(yt, F.quantize_ref(x, s_ref, fmt).t().contiguous(), tag + " codes", f"{r}x{c} current")
    e = C.fp8_quantize_t(torch.zeros(0, 8, dtype=dt, device=DEV), fmt, _scalar(1.0))
    assert e.shape == (8, 0)


# ----------------------------------------------------------------------------
# fp8_amax
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", F.IN_DTYPES, ids=DT_IDS)
def test_amax(dt):
    C = _C()
    tag = f"amax {F.DT_NAME[dt]}"
    for name, x in F.amax_cases(dt):
        xd = x.to(DEV)
        amax = torch.zeros(1, device=DEV)
        C.fp8_amax(xd, amax)
        print(f"{tag} {name}: {float(amax):g} (ref {F.amax_ref(x):g})")
        _val(amax, F.amax_ref(x), tag, name)
        amax = _scalar(1e6)
        C.fp8_amax(xd, amax)
        _val(amax, 1e6, tag, name + " pre-filled")
    amax = _scalar(0.25)
    C.fp8_amax(torch.zeros(0, dtype=dt, device=DEV), amax)
    _val(amax, 0.25, tag, "empty")


# ----------------------------------------------------------------------------
# fp8_quantize_weights
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", F.FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("dt", F.IN_DTYPES, ids=DT_IDS)
def test_quantize_weights(dt, fmt):
    """One call with a weight for every branch: against the reference, and bit-identical to the per-weight
    fp8_amax + fp8_quantize + fp8_quantize_t; unused slots keep their contents."""
    C = _C()
    ws = F.wq_weights(dt)
    wd = [w.to(DEV) for w in ws]
    want_t = [t for _, _, t in F.WQ_WEIGHTS]
    smax = F.FMT_MAX[fmt] * 0.5
    garbage = [torch.arange(F.WQ_NSLOTS, dtype=torch.float32) + v for v in (77.0, 88.0, 99.0)]
    scale, sinv, amax = (t.to(DEV) for t in garbage)
    outs = C.fp8_quantize_weights(wd, F.WQ_SLOTS, want_t, fmt, scale, sinv, amax, smax)
    assert len(outs) == 2 * len(ws)
    tag = f"quantize_weights {F.FMT_NAME[fmt]} {F.DT_NAME[dt]}"
    exp = [t.clone() for t in garbage]
    for i, (w, slot) in enumerate(zip(ws, F.WQ_SLOTS)):
        a = F.amax_ref(w)
        s_ref, sinv_ref = F.current_scale(a, smax)
        exp[0][slot], exp[1][slot], exp[2][slot] = s_ref, sinv_ref, a
        codes = F.quantize_ref(w, s_ref, fmt)
        what = f"weight {i} {tuple(w.shape)}"
        _same(outs[2 * i], codes, tag + " codes", what)
        if want_t[i]:
            _same(outs[2 * i + 1], codes.t().contiguous(), tag + " codes_t", what)
        else:
            assert outs[2 * i + 1].numel() == 0
        # the per-weight path
        a1, s1, i1 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        C.fp8_amax(wd[i], a1)
        y1 = C.fp8_quantize(wd[i], fmt, s1, None, a1, i1, smax)
        _same(outs[2 * i], y1, tag + " vs per-weight", what)
        if want_t[i]:
            yt1 = C.fp8_quantize_t(wd[i], fmt, torch.zeros(1, device=DEV), None, a1, torch.zeros(1, device=DEV), smax)
            _same(outs[2 * i + 1], yt1, tag + " vs per-weight", what + " t")
        assert float(s1) == float(scale[slot]) and float(i1) == float(sinv[slot]) and float(a1) == float(amax[slot])
    assert exp[0][F.WQ_SLOTS[F.WQ_ZERO]] == 1.0 and exp[2][F.WQ_SLOTS[F.WQ_ZERO]] == 0.0
    for name, got, want in zip(("scale", "scale_inv", "amax"), (scale, sinv, amax), exp):
        print(f"{tag} {name}: {got.cpu().tolist()}")
        _same(got, want, tag + " " + name)
    assert C.fp8_quantize_weights([], [], [], fmt, scale, sinv, amax, smax) == []


# ----------------------------------------------------------------------------
# fp8_update_scales
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("hist_len", [1, 16])
def test_update_scales(hist_len):
    """Three consecutive calls (the index wraps, margins 1, 0.5, 2**-3, inf / NaN amaxes, an all-zero window,
    n_slots below the buffers' size) against the reference state after each."""
    C = _C()
    (hist, amax, scale, sinv, fmax), calls = F.update_scales_scenario(hist_len)
    dev = [t.to(DEV) for t in (hist, amax, scale, sinv, fmax)]
    tag = f"update_scales L={hist_len}"
    for k, (a, idx, margin) in enumerate(calls):
        amax = a.clone()
        dev[1].copy_(a)
        hist, amax, scale, sinv = F.update_scales_ref(hist, amax, scale, sinv, fmax, F.US_N, idx, margin)
        C.fp8_update_scales(*dev, F.US_N, idx, margin)
        for name, got, want in zip(("hist", "amax_cur", "scale", "scale_inv"), dev, (hist, amax, scale, sinv)):
            bad = int((~((got.cpu() == want) | (torch.isnan(got.cpu()) & torch.isnan(want)))).sum())
            print(f"{tag} call {k} idx {idx} margin {margin:g} {name}: {bad} of {want.numel()} differ")
            _same(got, want, f"{tag} {name}", f"call {k}")
    assert bool(torch.isfinite(dev[0][:F.US_N]).all()) and bool(torch.isfinite(dev[2]).all())
    before = [t.clone() for t in dev]
    C.fp8_update_scales(*dev, 0, 0, 1.0)                              # no slots: nothing happens
    assert all(torch.equal(a.nan_to_num(nan=-1.0), b.nan_to_num(nan=-1.0)) for a, b in zip(before, dev))


# ----------------------------------------------------------------------------
# non-finite elements
# ----------------------------------------------------------------------------
def _nonfinite(dt, n, inf=True):
    x = (torch.arange(n, dtype=torch.float32) % 7 - 3.0) * 0.75
    x[1], x[n - 2] = float("nan"), float("nan")
    if inf:
        x[2], x[3], x[n - 1] = float("inf"), -float("inf"), float("inf")
    return x.to(dt)


@pytest.mark.parametrize("dt", F.IN_DTYPES, ids=DT_IDS)
def test_nonfinite_elements(dt):
    """What NaN and +-inf elements become, in the vector body and in the scalar tail: +-inf saturates to +-max and
    makes amax inf (which update_scales records as 0, test_update_scales); NaN is dropped by every amax and its
    code is F.NAN_CODE (-max: v_med3_f32 with a NaN operand returns the minimum of the other two)."""
    C = _C()
    n = 8 * 2 + 5
    for fmt in F.FMTS:
        tag = f"nonfinite {F.FMT_NAME[fmt]} {F.DT_NAME[dt]}"
        for inf in (True, False):
            x = _nonfinite(dt, n, inf)
            xd = x.to(DEV)
            want_amax = float("inf") if inf else 2.25
            assert F.amax_ref(x) == want_amax
            amax = torch.zeros(1, device=DEV)
            y = C.fp8_quantize(xd, fmt, _scalar(37.5), amax)
            print(f"{tag} inf={inf}: codes at NaN {[hex(v) for v in y.cpu()[[1, n - 2]].tolist()]}, at +inf -inf +inf "
                  f"{[hex(v) for v in y.cpu()[[2, 3, n - 1]].tolist()]}, amax {float(amax)}")
            _same(y, F.quantize_ref(x, 37.5, fmt), tag + " codes", f"quantize inf={inf}")
            _val(amax, want_amax, tag + " amax", f"quantize inf={inf}")
            assert y.cpu()[1] == F.NAN_CODE[fmt] == F.MAX_CODE[fmt] | 0x80
            if inf:
                assert y.cpu()[[2, 3]].tolist() == [F.MAX_CODE[fmt], F.MAX_CODE[fmt] | 0x80]
            amax = torch.zeros(1, device=DEV)
            C.fp8_amax(xd, amax)
            _val(amax, want_amax, tag + " amax", f"amax inf={inf}")
            # transposing quantiser (3 x 7: byte stores) and the batched weight quantiser (scale from a NaN-free amax)
            x2 = x.view(3, 7)
            amax = torch.zeros(1, device=DEV)
            yt = C.fp8_quantize_t(x2.to(DEV), fmt, _scalar(37.5), amax)
            _same(yt, F.quantize_ref(x2, 37.5, fmt).t().contiguous(), tag + " codes", f"quantize_t inf={inf}")
            _val(amax, want_amax, tag + " amax", f"quantize_t inf={inf}")
            scale, sinv, am = torch.zeros(2, device=DEV), torch.zeros(2, device=DEV), torch.zeros(2, device=DEV)
            yw, ywt = C.fp8_quantize_weights([x2.to(DEV)], [1], [True], fmt, scale, sinv, am, F.FMT_MAX[fmt])
            s_ref, sinv_ref = F.current_scale(want_amax, F.FMT_MAX[fmt])
            assert (s_ref == 1.0) == inf
            _val(am[1:], want_amax, tag + " amax", f"quantize_weights inf={inf}")
            _val(scale[1:], s_ref, tag + " scale", f"quantize_weights inf={inf}")
            _same(yw, F.quantize_ref(x2, s_ref, fmt), tag + " codes", f"quantize_weights inf={inf}")
            _same(ywt, F.quantize_ref(x2, s_ref, fmt).t().contiguous(), tag + " codes", f"quantize_weights t inf={inf}")


def test_amp_skips_an_overflowed_step_with_fp8():
    """amp O2 with fp8 on, dynamic loss scale: a step whose loss is infinite (every gradient that reaches a bias,
    a LayerNorm or an embedding is inf or NaN, while the fp8 quantisers saturate what they are given) is skipped
    by the overflow check — no parameter moves, the loss scale drops, the fp8 scales stay finite — and the next
    step trains."""
    from apex import amp, fp8
    from apex.amp._amp_state import _amp_state
    from apex.models.bert import BertConfig, BertForPreTraining, synthetic_batch
    from apex.optimizers import FusedAdam

    _amp_state.optimizers, _amp_state.loss_scalers = [], []
    fp8.disable()
    try:
        torch.manual_seed(5)
        cfg = BertConfig(vocab_size=512, hidden_size=256, num_hidden_layers=1, num_attention_heads=4,
                         intermediate_size=1024, max_position_embeddings=128, hidden_dropout_prob=0.0,
                         attention_probs_dropout_prob=0.0)
        model = BertForPreTraining(cfg).to(DEV)
        opt = FusedAdam(model.parameters(), lr=1e-3)
        model, opt = amp.initialize(model, opt, opt_level="O2", cast_model_type=torch.bfloat16, verbosity=0,
                                    fp8=True, loss_scale="dynamic")
        scaler = _amp_state.loss_scalers[0]
        assert scaler.dynamic
        batch = synthetic_batch(cfg, 8, 128, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))

        def step(poison):
            loss = model(**batch)
            with amp.scale_loss(loss * float("inf") if poison else loss, opt) as sl:
                sl.backward()
            bad = sum(int((~torch.isfinite(p.grad)).sum()) for p in model.parameters() if p.grad is not None)
            opt.step()
            opt.zero_grad()
            return float(loss), bad

        l0, bad0 = step(False)
        st = fp8.state()
        assert st.n >= 4 * 3 and bad0 == 0
        before = [p.detach().clone() for p in model.parameters()]
        scale_before = scaler.loss_scale()
        _, bad1 = step(True)
        moved = sum(int((p.detach() != q).sum()) for p, q in zip(model.parameters(), before))
        print(f"poisoned step: {bad1} non-finite gradient elements, {moved} parameter elements moved, loss scale "
              f"{scale_before} -> {scaler.loss_scale()}")
        assert bad1 > 0 and moved == 0
        assert scaler.loss_scale() < scale_before
        n = st.n
        for name in ("scale", "scale_inv", "hist", "amax"):
            t = getattr(st, name)[:n]
            assert bool(torch.isfinite(t).all()), name
        assert bool((st.scale[:n] > 0).all())
        l2, bad2 = step(False)
        moved = sum(int((p.detach() != q).sum()) for p, q in zip(model.parameters(), before))
        print(f"losses {l0:.4f} -> {l2:.4f}; after the next step {moved} parameter elements moved")
        assert l2 == l2 and abs(l2) != float("inf") and bad2 == 0 and moved > 0
    finally:
        fp8.disable()
        _amp_state.optimizers, _amp_state.loss_scalers = [], []


# ----------------------------------------------------------------------------
# gemm_f8
# ----------------------------------------------------------------------------
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _gemm_f8(epi, A8, B8, aa, ab, fa, T, bias=None, aux=None, bdt=None, **kw):
    C = _C()
    return C.gemm_f8(A8, B8, _scalar(aa), _scalar(ab), fa, getattr(C, R.epi_attr(epi)), bias if R.has_bias(epi) else None,
                     aux if R.aux_in(epi) else None, bdt if R.colsum(epi) else None, T, **kw)


def _device_a(shape, A8):
    Ad = A8.to(DEV)
    if shape.layout == "lda":       # a column slice of a wider matrix: lda = K + 128, a multiple of 16
        wide = torch.full((shape.M, shape.K + 128), 0x38, dtype=torch.uint8, device=DEV)
        wide[:, 64:64 + shape.K] = Ad
        Ad = wide[:, 64:64 + shape.K]
        assert Ad.stride(0) == shape.K + 128 and not Ad.is_contiguous() and Ad.data_ptr() % 16 == 0
    elif shape.layout == "a3d":
        Ad = Ad.view(2, shape.M // 2, shape.K)
    return Ad


_EXACT_EXPECTED = {}


def _exact_expected(shape, fa):
    """Codes and the int64 results of gemm_reference.EXACT_EPIS from one gathered product (the small shapes are
    held to gemm_reference.exact_expected, which gathers once per epilogue)."""
    key = (shape.M, shape.N, shape.K, fa)
    if key not in _EXACT_EXPECTED:
        A8, B8, A, B, bias, aux = F.exact_operands(shape.M, shape.N, shape.K, fa)
        acc = R.exact_acc(A, B)
        mul = acc * aux
        exp = {"none": {"C": acc}, "bias": {"C": acc + bias[None, :]}, "resid": {"C": acc + aux},
               "mul": {"C": mul, "dbias": mul.sum(0)}, "bias_gelu": {"X": acc + bias[None, :]}}
        assert set(exp) == set(R.EXACT_EPIS)
        if shape.M * shape.N <= 512 * 512:
            for e in R.EXACT_EPIS:
                ref = R.exact_expected(e, A, B, bias, aux)
                assert ref.keys() == exp[e].keys() and all(torch.equal(ref[k], exp[e][k]) for k in ref), e
        _EXACT_EXPECTED.clear()      # (one shape's int64 tables at a time)
        _EXACT_EXPECTED[key] = (A8, B8, bias, aux, exp)
    return _EXACT_EXPECTED[key]


def _exact(shape, fa, persist, epis=tuple(R.EXACT_EPIS)):
    C = _C()
    C.set_gemm_persist(1, 1 if persist else 0)
    A8, B8, bias, aux, exp = _exact_expected(shape, fa)
    Ad, Bd = _device_a(shape, A8), B8.to(DEV)
    for T in R.DTYPES:
        bd, xd = bias.to(T).to(DEV), aux.to(T).to(DEV)
        tag = f"gemm_f8 exact {shape.path} {F.FMT_NAME[fa]} {F.DT_NAME[T]}"
        for epi in epis:
            c, x = _gemm_f8(epi, Ad, Bd, *F.EXACT_ALPHA, fa, T, bd, xd, F32)
            assert c.dtype == T and c.shape[:-1] == Ad.shape[:-1] and c.shape[-1] == shape.N
            for name, want in exp[epi].items():
                got = (c if name == "C" else x).reshape(want.shape).double()
                bad = int((got.cpu() != want.double()).sum())
                print(f"{shape.name} {F.FMT_NAME[fa]} {F.DT_NAME[T]} exact {epi} {name}: {bad} of {want.numel()} differ")
                _same(got, want.double(), tag, f"{shape.name} {epi} {name}")


_ACC = {}


def _dense_case(shape, fa, T, on_device=False):
    """Operands of one dense case and its float64 product (computed once per shape and format, left unchanged)."""
    key = (shape.name, fa, on_device)
    if key not in _ACC:
        ops = F.dense_code_operands(shape.name, shape.M, shape.N, shape.K, fa)
        A8, B8 = (ops[0].to(DEV), ops[1].to(DEV)) if on_device else ops[:2]
        _ACC.clear()
        _ACC[key] = (ops, F.acc_ref(A8, B8, fa, F.E4M3, F.alpha_of(ops[2], ops[3])))
    ops, ref = _ACC[key]
    return (*ops, *F.dense_bias_aux(shape.name, shape.M, shape.N, T)), ref


def _dense(shape, fa, persist, epis=tuple(R.EPIS), on_device=False):
    """Every epilogue, output dtype and bias-gradient dtype of one shape and format against the bound."""
    C = _C()
    C.set_gemm_persist(1, 1 if persist else 0)
    for T in R.DTYPES:
        (A8, B8, aa, ab, bias, aux), (acc, cond) = _dense_case(shape, fa, T, on_device)
        Ad, Bd, bd, xd = _device_a(shape, A8), B8.to(DEV), bias.to(DEV), aux.to(DEV)
        if on_device:
            bias, aux = bd, xd
        for epi in epis:
            for bdt in ((F32, T) if R.colsum(epi) else (None,)):
                c, x = _gemm_f8(epi, Ad, Bd, aa, ab, fa, T, bd, xd, bdt)
                assert c.shape[:-1] == Ad.shape[:-1] and c.shape[-1] == shape.N
                r = F.check_epilogue(epi, T, shape.K, acc, cond, c, x, bias, aux, bdt,
                                     what=f"{shape.name} {F.FMT_NAME[fa]} {F.DT_NAME[T]}",
                                     tag=f"gemm_f8 {shape.path} {F.FMT_NAME[fa]}")
                CASES["n"] += 1
                print(f"{shape.name} {F.FMT_NAME[fa]} {F.DT_NAME[T]} {epi} db={F.DT_NAME[bdt]}: worst error / bound {r:.3f}")
                if epi == "none":
                    m = _acc_measure(f"gemm_f8 none -> {F.DT_NAME[T]}", c.reshape(acc.shape), acc, cond,
                                     F.HALF_ULP[T] + F.E24, F.TINY[T])
                    print(f"{shape.name} {F.FMT_NAME[fa]} {F.DT_NAME[T]}: worst |err| / (2**-24 cond) {m:.1f}")


@pytest.mark.parametrize("fa", F.FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("shape", F.NT_SHAPES, ids=[s.name for s in F.NT_SHAPES])
def test_gemm_exact(shape, fa):
    _exact(shape, fa, persist=False)


@pytest.mark.parametrize("fa", F.FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("shape", F.NT_SHAPES, ids=[s.name for s in F.NT_SHAPES])
def test_gemm_dense(shape, fa):
    _dense(shape, fa, persist=False)


def _persist_shape(K):
    cus = _cus()
    shape = F.persist_shape(cus, K)
    tiles = (shape.M // 256) * (shape.N // 256)
    print(f"{cus} CUs, {tiles} full tiles")
    assert tiles > cus
    return shape


@pytest.mark.parametrize("fa", F.FMTS, ids=FMT_IDS)
def test_gemm_persistent_exact(fa):
    _exact(_persist_shape(256), fa, persist=True)


@pytest.mark.parametrize("fa", F.FMTS, ids=FMT_IDS)
def test_gemm_persistent_dense(fa):
    _dense(_persist_shape(384), fa, persist=True, epis=("bias", "bias_gelu", "bias_gelu_tanh_d", "dgelu"), on_device=True)


@pytest.mark.parametrize("fa", F.FMTS, ids=FMT_IDS)
def test_gemm_persistent_matches_one_tile_bitwise(fa):
    """Every epilogue, with and without the Q8 side output: the same bits from both kernels in C, in the second
    output (H, gelu' or the fp32 bias gradient), in the codes and in amax; the bias gradient of each kernel is also
    held to the bias-gradient bound of the dh it stored. (With fp16 output and the dGELU epilogues writing Q8 codes
    the persistent kernel's bias gradient used to differ in 140 of 1024 columns: its column sums took elements 0
    and 1 of a chunk from a separately rounded product, csrc/gemm_epilogue.h.)"""
    C = _C()
    shape = _persist_shape(128)
    T = BF16 if fa == F.E4M3 else F16
    A8, B8, aa, ab, bias, aux = (t.to(DEV) if isinstance(t, torch.Tensor) else t
                                 for t in F.dense_operands(shape.name, shape.M, shape.N, shape.K, fa, T))
    for epi in R.EPIS:
        for q8 in ((False, True) if epi in F.Q8_EPIS else (False,)):
            outs = []
            for persist in (0, 1):
                C.set_gemm_persist(1, persist)
                kw, amax = {}, torch.zeros(1, device=DEV)
                if q8:
                    kw = dict(q8_out=torch.zeros(shape.M, shape.N, dtype=torch.uint8, device=DEV), q8_scale=_scalar(23.7),
                              q8_amax=amax, q8_fmt=fa)
                c, x = _gemm_f8(epi, A8, B8, aa, ab, fa, T, bias, aux, F32, **kw)
                outs.append((c, x, kw.get("q8_out"), amax))
            tag = f"gemm_f8 persist vs one-tile {F.FMT_NAME[fa]}"
            _same(outs[1][0], outs[0][0], tag, f"{epi} q8={q8} C")
            if R.colsum(epi):
                for k, kernel in enumerate(("one-tile", "persistent")):
                    ref, bound = R.bias_grad_expected(outs[k][0], F32)
                    r = R.check(outs[k][1], ref, bound, f"{epi} q8={q8} {kernel} bias gradient",
                                f"gemm_f8 {kernel} {F.FMT_NAME[fa]} {epi} dbias f32")
                differ = int((outs[1][1] != outs[0][1]).sum())
                print(f"{epi} q8={q8} {F.DT_NAME[T]}: worst bias-gradient error / bound {r:.3f}; {differ} of {shape.N} "
                      f"elements differ between the kernels")
            if outs[0][1] is not None and outs[0][1].numel():
                _same(outs[1][1], outs[0][1], tag, f"{epi} q8={q8} X")
            if q8:
                _same(outs[1][2], outs[0][2], tag, f"{epi} codes")
                _same(outs[1][3], outs[0][3], tag, f"{epi} amax")
                assert float(outs[0][3]) > 0


# ----------------------------------------------------------------------------
# Q8 side outputs
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("q8_fmt", F.FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("shape", F.Q8_SHAPES, ids=[s.name for s in F.Q8_SHAPES])
def test_gemm_q8_side_output(shape, q8_fmt):
    """Codes = the reference's encoding of the C the kernel stored, amax = max |C| exactly (on the edge shape with
    F.phantom_last_column's trap for the lanes past N); a larger pre-filled amax stays; q8_only gives the same
    codes and second output. The GELU forwards run with e4m3 A, the gradient epilogues with e5m2 A."""
    M, N = shape.M, shape.N
    for T in R.DTYPES:
        for epi in F.Q8_EPIS:
            fa = F.E4M3 if R.gelu_fwd(epi) else F.E5M2
            A8, B8, aa, ab, bias, aux = F.dense_operands(shape.name, M, N, shape.K, fa, T)
            if shape.path == "edge":
                big = F.phantom_last_column(A8, B8, bias, fa)
                assert big > 20.0
            Ad, Bd, bd, xd = A8.to(DEV), B8.to(DEV), bias.to(DEV), aux.to(DEV)
            tag = f"gemm_f8 q8 {shape.path} {F.FMT_NAME[q8_fmt]} {F.DT_NAME[T]}"
            what = f"{shape.name} {epi}"
            plain_c, plain_x = _gemm_f8(epi, Ad, Bd, aa, ab, fa, T, bd, xd, F32)
            q8_scale = F.f32(0.37 * F.FMT_MAX[q8_fmt] / max(F.amax_ref(plain_c.cpu()), 1e-3))
            codes = torch.full((M, N), 0x55, dtype=torch.uint8, device=DEV)
            amax = torch.zeros(1, device=DEV)
            kw = dict(q8_out=codes, q8_scale=_scalar(q8_scale), q8_amax=amax, q8_fmt=q8_fmt)
            c, x = _gemm_f8(epi, Ad, Bd, aa, ab, fa, T, bd, xd, F32, **kw)
            _same(c, plain_c, tag + " C", what)                       # the side output changes nothing else
            _same(x, plain_x, tag + " X", what)
            ref_codes, ref_amax = F.q8_expected(c.cpu(), q8_scale, q8_fmt)
            print(f"{what} {F.DT_NAME[T]} q8 {F.FMT_NAME[q8_fmt]}: {int((codes.cpu() != ref_codes).sum())} codes differ, "
                  f"amax {float(amax)!r} (ref {ref_amax!r})")
            _same(codes, ref_codes, tag + " codes", what)
            _val(amax, ref_amax, tag + " amax", what)
            # a larger pre-filled amax stays
            kw["q8_amax"] = _scalar(F.f32(3.0 * ref_amax + 1.0))
            _gemm_f8(epi, Ad, Bd, aa, ab, fa, T, bd, xd, F32, **kw)
            _val(kw["q8_amax"], F.f32(3.0 * ref_amax + 1.0), tag + " amax", what + " pre-filled")
            # codes only
            codes2 = torch.full((M, N), 0x55, dtype=torch.uint8, device=DEV)
            amax2 = torch.zeros(1, device=DEV)
            kw = dict(q8_out=codes2, q8_scale=_scalar(q8_scale), q8_amax=amax2, q8_fmt=q8_fmt, q8_only=True)
            _, x2 = _gemm_f8(epi, Ad, Bd, aa, ab, fa, T, bd, xd, F32, **kw)
            _same(codes2, codes, tag + " codes", what + " q8_only")
            _same(x2, x, tag + " X", what + " q8_only")
            _same(amax2, amax, tag + " amax", what + " q8_only")


# ----------------------------------------------------------------------------
# gemm_tt_f8
# ----------------------------------------------------------------------------
def _slot(P, Q, dtype):
    """A [P, Q] slot 16 bytes into a larger guarded buffer."""
    off = 16 // torch.empty((), dtype=dtype).element_size()
    guard = torch.full((P * Q + 2 * off + 64,), GUARD, dtype=dtype, device=DEV)
    return guard, guard[off:off + P * Q].view(P, Q), off


def _guard_ok(guard, off, n):
    g = guard.cpu().float()
    return bool((g[:off] == GUARD).all()) and bool((g[off + n:] == GUARD).all())


@pytest.mark.parametrize("fa", F.FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("case", F.WGRAD, ids=[f"r{r}-{p}x{q}-s{s}" for (r, p, q, s) in F.WGRAD])
def test_wgrad(case, fa):
    C = _C()
    Rr, P, Q, s = case
    # integer case: bit-exact in every output dtype, into a guarded slot too
    E8, G8, A, B, _, _ = F.exact_operands(P, Q, Rr, fa)
    want = R.exact_acc(A, B).double()
    a8, b8 = E8.t().contiguous().to(DEV), G8.t().contiguous().to(DEV)
    assert C.gemm_tt_f8_supported(a8, b8, s)
    al = [_scalar(v) for v in F.EXACT_ALPHA]
    for odt in (F32, BF16, F16):
        guard, slot, off = _slot(P, Q, odt)
        tag = f"gemm_tt_f8 exact {F.FMT_NAME[fa]}->{F.DT_NAME[odt]}"
        _same(C.gemm_tt_f8(a8, b8, *al, fa, 0, s, odt).double(), want, tag, f"{case}")
        out = C.gemm_tt_f8(a8, b8, *al, fa, 0, s, odt, out=slot)
        assert out.data_ptr() == slot.data_ptr()
        _same(out.double(), want, tag, f"{case} slot")
        assert _guard_ok(guard, off, P * Q), "guard band written"
    # dense case
    A8, B8, aa, ab = F.dense_wgrad_operands(f"{Rr}x{P}x{Q}", Rr, P, Q, fa)
    Ad, Bd = A8.to(DEV), B8.to(DEV)
    for odt in (F32, BF16, F16):
        ref, bound = F.wgrad_expected(A8, B8, fa, F.E4M3, F.alpha_of(aa, ab), s, odt)
        out = C.gemm_tt_f8(Ad, Bd, _scalar(aa), _scalar(ab), fa, 0, s, odt)
        assert out.dtype == odt and out.shape == (P, Q)
        r = R.check(out, ref, bound, f"wgrad f8 r{Rr} {P}x{Q} s{s} -> {F.DT_NAME[odt]}",
                    f"gemm_tt_f8 {F.FMT_NAME[fa]}->{F.DT_NAME[odt]}")
        CASES["n"] += 1
        print(f"wgrad f8 r{Rr} {P}x{Q} s{s} {F.FMT_NAME[fa]} -> {F.DT_NAME[odt]}: worst error / bound {r:.3f}")
        if odt == F32:
            a64, b64 = F.decode(A8, fa), F.decode(B8, F.E4M3)
            cond = abs(F.alpha_of(aa, ab)) * (a64.abs().t() @ b64.abs())
            m = _acc_measure("gemm_tt_f8 -> f32", out, ref, cond)
            print(f"wgrad f8 r{Rr} {P}x{Q} s{s} {F.FMT_NAME[fa]}: worst |err| / (2**-24 cond) {m:.1f}")


# ----------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------
def _misaligned(t):
    """t's values, contiguous, at a data pointer one element past 16-byte alignment."""
    flat = torch.empty(t.numel() + 16, dtype=t.dtype, device=DEV)
    flat[1:1 + t.numel()] = t.reshape(-1).to(DEV)
    v = flat[1:1 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def _refused(fn, *args, **kw):
    with pytest.raises(RuntimeError):
        fn(*args, **kw)
    CASES["n"] += 1


@pytest.mark.parametrize("dt", F.IN_DTYPES, ids=DT_IDS)
def test_quantizer_refusals(dt):
    """fp8_quantize / fp8_quantize_t / fp8_amax / fp8_quantize_weights: every operand that the kernels cannot take
    raises before a launch (the outputs given keep their contents)."""
    C = _C()
    x = torch.randn(64, 72).to(dt)
    xd = x.to(DEV)
    one = _scalar(1.0)
    amax, sinv = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    for q in (C.fp8_quantize, C.fp8_quantize_t):
        _refused(q, x, 0, one)                                         # a CPU input
        _refused(q, xd.double(), 0, one)                               # a dtype outside bf16 / fp16 / fp32
        _refused(q, xd.to(torch.int32), 0, one)
        _refused(q, _misaligned(x), 0, one)                            # a contiguous view at an odd element offset
        _refused(q, xd.t(), 0, one)                                    # not contiguous
        _refused(q, xd, 2, one)                                        # fmt
        _refused(q, xd, -1, one)
        _refused(q, xd, 0, torch.ones(1))                              # a CPU scale
        _refused(q, xd, 0, torch.ones(1, dtype=torch.float64, device=DEV))
        _refused(q, xd, 0, torch.ones(0, device=DEV))
        _refused(q, xd, 0, one, torch.zeros(1))                        # a CPU amax
        _refused(q, xd, 0, one, amax.half())
        _refused(q, xd, 0, one, None, torch.ones(1), sinv, 448.0)      # a CPU cur_amax
        _refused(q, xd, 0, one, None, amax, torch.ones(1), 448.0)      # a CPU scale_inv
        _refused(q, xd, 0, one, None, amax, None, 448.0)               # current scaling without scale_inv
        _refused(q, xd, 0, one, None, amax, sinv, 0.0)                 # smax
    _refused(C.fp8_quantize_t, xd.view(-1), 0, one)                    # not 2-D
    _refused(C.fp8_amax, x, amax)
    _refused(C.fp8_amax, xd.double(), amax)
    _refused(C.fp8_amax, _misaligned(x), amax)
    _refused(C.fp8_amax, xd.t(), amax)
    _refused(C.fp8_amax, xd, torch.zeros(1))
    _refused(C.fp8_amax, xd, amax.double())
    _refused(C.fp8_amax, xd, amax[:0])
    assert float(amax) == 0.0 and float(sinv) == 0.0 and float(one) == 1.0
    # accepted: an aligned offset view
    flat = torch.zeros(64 * 72 + 8, dtype=dt, device=DEV)
    C.fp8_quantize(flat[16 // flat.element_size():][:64 * 72 - 8], 0, one)

    sc, si, am = (torch.full((4,), 5.0, device=DEV) for _ in range(3))
    qw = C.fp8_quantize_weights
    ok = ([xd], [1], [True], 0, sc, si, am, 448.0)
    qw(*ok)
    sc.fill_(5.0), si.fill_(5.0), am.fill_(5.0)
    _refused(qw, [x], [1], [True], 0, sc, si, am, 448.0)               # a CPU weight
    _refused(qw, [_misaligned(x)], [1], [True], 0, sc, si, am, 448.0)
    _refused(qw, [xd.t()], [1], [True], 0, sc, si, am, 448.0)
    _refused(qw, [xd.view(-1)], [1], [True], 0, sc, si, am, 448.0)
    _refused(qw, [xd.double()], [1], [True], 0, sc, si, am, 448.0)
    _refused(qw, [xd, xd.to(F32 if dt != F32 else BF16)], [1, 2], [True, True], 0, sc, si, am, 448.0)   # mixed dtypes
    _refused(qw, [xd], [4], [True], 0, sc, si, am, 448.0)              # slot out of range
    _refused(qw, [xd], [-1], [True], 0, sc, si, am, 448.0)
    _refused(qw, [xd], [1, 2], [True], 0, sc, si, am, 448.0)           # one slot per weight
    _refused(qw, [xd], [1], [True, False], 0, sc, si, am, 448.0)
    _refused(qw, [xd], [1], [True], 2, sc, si, am, 448.0)              # fmt
    _refused(qw, [xd], [1], [True], 0, sc, si, am, 0.0)                # smax
    _refused(qw, [xd], [1], [True], 0, sc.cpu(), si, am, 448.0)
    _refused(qw, [xd], [1], [True], 0, sc, si.cpu(), am, 448.0)        # scale_inv not on the device
    _refused(qw, [xd], [1], [True], 0, sc, si, am.cpu(), 448.0)        # amax not on the device
    _refused(qw, [xd], [1], [True], 0, sc, si.double(), am, 448.0)
    _refused(qw, [xd], [1], [True], 0, sc, si, am[:1], 448.0)          # amax shorter than the slot
    _refused(qw, [xd], [1], [True], 0, sc, torch.zeros(8, device=DEV)[::2], am, 448.0)
    assert all(bool((t == 5.0).all()) for t in (sc, si, am))


def test_update_scales_refusals():
    C = _C()
    n, L = 6, 4
    mk = lambda: torch.full((n,), 2.0, device=DEV)  # noqa: E731
    hist, amax, scale, sinv, fmax = torch.zeros(n, L, device=DEV), mk(), mk(), mk(), mk()
    us = C.fp8_update_scales
    us(hist, amax, scale, sinv, fmax, n, 0, 1.0)
    amax.fill_(2.0)
    _refused(us, hist, amax, scale, sinv, fmax, -1, 0, 1.0)            # n_slots out of range
    _refused(us, hist, amax, scale, sinv, fmax, n + 1, 0, 1.0)
    _refused(us, hist, amax, scale, sinv, fmax, n, L, 1.0)             # index out of range
    _refused(us, hist, amax, scale, sinv, fmax, n, -1, 1.0)
    _refused(us, hist.cpu(), amax, scale, sinv, fmax, n, 0, 1.0)
    _refused(us, hist.double(), amax, scale, sinv, fmax, n, 0, 1.0)
    _refused(us, hist.view(-1), amax, scale, sinv, fmax, n, 0, 1.0)
    _refused(us, hist.t(), amax, scale, sinv, fmax, L, 0, 1.0)
    for i in range(1, 5):                                              # amax_cur, scale, scale_inv, fmt_max in turn
        for bad in (lambda t: t.cpu(), lambda t: t.double(), lambda t: t[:n - 1], lambda t: torch.cat([t, t])[::2]):
            args = [hist, amax, scale, sinv, fmax]
            args[i] = bad(args[i])
            _refused(us, *args, n, 0, 1.0)
    assert bool((amax == 2.0).all())                                   # nothing ran
    us(hist, amax, scale, sinv, fmax, n - 1, 0, 1.0)                   # fewer slots than the buffers hold: fine
    assert float(amax[n - 1]) == 2.0 and float(amax[0]) == 0.0


@pytest.mark.parametrize("T", R.DTYPES, ids=DT_IDS)
def test_gemm_f8_refusals(T):
    C = _C()
    M, N, K = 256, 264, 128
    A8, B8, aa, ab, bias, aux = F.dense_operands("reject", M, N, K, F.E4M3, T)
    Ad, Bd, bd, xd = A8.to(DEV), B8.to(DEV), bias.to(DEV), aux.to(DEV)
    sa, sb = _scalar(aa), _scalar(ab)
    assert C.gemm_f8_supported(Ad, Bd)
    for a, b in ((Ad, B8), (A8, Bd), (Ad, _misaligned(B8)), (_misaligned(A8), Bd), (Ad, Bd[:, :K - 16]), (Ad.char(), Bd),
                 (Ad, Bd.char()), (Ad, Bd[:N - 4]), (Ad.view(-1), Bd), (Ad[:, ::2], Bd[:, ::2]),
                 (torch.zeros(64, 100, dtype=torch.uint8, device=DEV), torch.zeros(64, 100, dtype=torch.uint8, device=DEV))):
        assert not C.gemm_f8_supported(a, b)
        _refused(C.gemm_f8, a, b, sa, sb, 0, C.EPI_NONE, None, None, None, T)

    def refused(*args, **kw):
        _refused(C.gemm_f8, Ad, Bd, *args, **kw)

    refused(sa.cpu(), sb, 0, C.EPI_NONE, None, None, None, T)                       # CPU alpha
    refused(sa, sb.cpu(), 0, C.EPI_NONE, None, None, None, T)
    refused(sa.double(), sb, 0, C.EPI_NONE, None, None, None, T)
    refused(sa, sb[:0], 0, C.EPI_NONE, None, None, None, T)
    refused(sa, sb, 2, C.EPI_NONE, None, None, None, T)                             # fmt_a
    valid = {getattr(C, R.epi_attr(e)) for e in R.EPIS}
    (f32_slab,) = set(range(C.EPI_MUL + 1)) - valid                                 # (the weight gradient's own epilogue)
    refused(sa, sb, 0, f32_slab, None, None, None, T)                               # epilogue codes
    refused(sa, sb, 0, C.EPI_MUL + 1, None, None, None, T)
    refused(sa, sb, 0, 99, None, None, None, T)
    refused(sa, sb, 0, -1, None, None, None, T)
    refused(sa, sb, 0, C.EPI_NONE, None, None, None, F32)                           # out_dtype
    other = F16 if T == BF16 else BF16
    refused(sa, sb, 0, C.EPI_BIAS, None, None, None, T)                             # bias missing
    refused(sa, sb, 0, C.EPI_BIAS, bias, None, None, T)                             # CPU bias
    refused(sa, sb, 0, C.EPI_BIAS_GELU, _misaligned(bias), None, None, T)
    refused(sa, sb, 0, C.EPI_BIAS_GELU_D, bd[:N - 8], None, None, T)
    refused(sa, sb, 0, C.EPI_BIAS_GELU_TANH, torch.cat([bd, bd])[::2], None, None, T)
    refused(sa, sb, 0, C.EPI_BIAS, bd.to(other), None, None, T)
    refused(sa, sb, 0, C.EPI_RESID, None, None, None, T)                            # aux missing
    refused(sa, sb, 0, C.EPI_RESID, None, aux, None, T)                             # CPU aux
    refused(sa, sb, 0, C.EPI_MUL, None, _misaligned(aux), F32, T)
    refused(sa, sb, 0, C.EPI_DGELU, None, xd[:M - 1], F32, T)
    refused(sa, sb, 0, C.EPI_DGELU_TANH, None, xd.t(), F32, T)
    refused(sa, sb, 0, C.EPI_MUL, None, xd.to(other), F32, T)
    refused(sa, sb, 0, C.EPI_MUL, None, xd, torch.float64, T)                       # bias_grad_dtype
    codes, amax, qs = torch.zeros(M, N, dtype=torch.uint8, device=DEV), torch.zeros(1, device=DEV), _scalar(3.0)
    q = dict(q8_out=codes, q8_scale=qs, q8_amax=amax, q8_fmt=0)
    refused(sa, sb, 0, C.EPI_BIAS, bd, None, None, T, **q)                          # no codes from this epilogue
    refused(sa, sb, 0, C.EPI_BIAS_GELU, bd, None, None, T, q8_only=True)            # q8_only without q8_out
    for k, v in (("q8_out", codes.cpu()), ("q8_out", codes[:M - 1]), ("q8_out", codes.char()),
                 ("q8_out", _misaligned(codes.cpu())), ("q8_out", torch.zeros(M, 2 * N, dtype=torch.uint8, device=DEV)[:, ::2]),
                 ("q8_scale", qs.cpu()), ("q8_scale", qs.double()), ("q8_scale", None), ("q8_amax", amax.cpu()),
                 ("q8_amax", amax.half()), ("q8_amax", None), ("q8_fmt", 2), ("q8_fmt", -1)):
        refused(sa, sb, 0, C.EPI_BIAS_GELU, bd, None, None, T, **{**q, k: v})
    assert float(amax) == 0.0 and int(codes.max()) == 0
    # an empty product (M = 0, N = 0, K = 0) is refused, not answered with an empty tensor
    for a, b in ((Ad[:0], Bd), (Ad, Bd[:0]), (Ad[:, :0], Bd[:, :0]), (Ad.view(2, M // 2, K)[:0], Bd)):
        assert a.numel() == 0 or b.numel() == 0
        assert not C.gemm_f8_supported(a, b)
        _refused(C.gemm_f8, a, b, sa, sb, 0, C.EPI_NONE, None, None, None, T)
    # accepted: the plain call
    c, _ = C.gemm_f8(Ad, Bd, sa, sb, 0, C.EPI_BIAS_GELU, bd, None, None, T, **q)
    assert float(amax) > 0.0


def test_gemm_tt_f8_refusals():
    C = _C()
    Rr, P, Q = 256, 256, 272
    a = F.dense_codes("tt-reject-a", Rr, P, F.E5M2).to(DEV)
    b = F.dense_codes("tt-reject-b", Rr, Q, F.E4M3).to(DEV)
    one = _scalar(1.0)
    assert C.gemm_tt_f8_supported(a, b, 2)
    for x, y, s in ((a, b.cpu(), 2), (a.cpu(), b, 2), (a, _misaligned(b.cpu()), 2), (_misaligned(a.cpu()), b, 2), (a, b, 0),
                    (a, b, 3), (a, b[:128], 1), (a.char(), b, 1), (a, b.char(), 1), (a[:, :P - 8], b, 1), (a, b[:, ::2], 1),
                    (a.view(-1), b, 1)):
        assert not C.gemm_tt_f8_supported(x, y, s)
        _refused(C.gemm_tt_f8, x, y, one, one, 1, 0, s, F32)
    tt = C.gemm_tt_f8
    # an empty product (R = 0, P = 0, Q = 0) is refused, not answered with an empty tensor
    for x, y in ((a[:0], b[:0]), (a[:, :0], b), (a, b[:, :0])):
        assert not C.gemm_tt_f8_supported(x, y, 1)
        _refused(tt, x, y, one, one, 1, 0, 1, F32)
    _refused(tt, a, b, one.cpu(), one, 1, 0, 2, F32)
    _refused(tt, a, b, one, one.cpu(), 1, 0, 2, F32)
    _refused(tt, a, b, one.double(), one, 1, 0, 2, F32)
    _refused(tt, a, b, one, one[:0], 1, 0, 2, F32)
    _refused(tt, a, b, one, one, 2, 0, 2, F32)                          # fmt_a
    _refused(tt, a, b, one, one, 1, 1, 2, F32)                          # fmt_b
    _refused(tt, a, b, one, one, 1, 0, 2, torch.float64)                # out_dtype
    # out: refused before the GEMM runs
    _refused(tt, a, b, one, one, 1, 0, 2, F32, out=torch.zeros(P, Q))
    _refused(tt, a, b, one, one, 1, 0, 2, F32, out=_misaligned(torch.zeros(P, Q)))
    _refused(tt, a, b, one, one, 1, 0, 2, F32, out=torch.zeros(P, Q, dtype=BF16, device=DEV))
    _refused(tt, a, b, one, one, 1, 0, 2, BF16, out=torch.zeros(P, Q, device=DEV))
    _refused(tt, a, b, one, one, 1, 0, 2, F32, out=torch.zeros(P, Q + 16, device=DEV))
    _refused(tt, a, b, one, one, 1, 0, 2, F32, out=torch.zeros(P, 2 * Q, device=DEV)[:, ::2])


def test_wrappers_copy_what_the_bindings_refuse():
    """Fp8State with a weight and an activation that are contiguous views at an odd element offset: the
    quantisers get aligned copies, and the results are those of the aligned tensors."""
    from apex import fp8

    st = fp8.Fp8State(device=DEV)
    g = R._gen("wrapper-misaligned")
    w = (torch.randn(264, 256, generator=g) * 0.05).to(BF16)
    x = torch.randn(64, 256, generator=g).to(BF16)
    wm, xm = _misaligned(w), _misaligned(x)
    w8, _ = st.weight(wm)
    wt8, _ = st.weight_t(wm)
    x8, _ = st.quantize(xm, (st.key_of(wm), "x"), fp8.E4M3)
    st2 = fp8.Fp8State(device=DEV)
    wa, xa = w.to(DEV), x.to(DEV)
    w8a, _ = st2.weight(wa)
    wt8a, _ = st2.weight_t(wa)
    x8a, _ = st2.quantize(xa, (st2.key_of(wa), "x"), fp8.E4M3)
    assert torch.equal(w8, w8a) and torch.equal(wt8, wt8a) and torch.equal(x8, x8a)
    s_ref, _ = F.current_scale(F.amax_ref(w), 448.0)
    _same(w8, F.quantize_ref(w, s_ref, F.E4M3), "wrappers misaligned", "weight")
    # the batched weight pass of the next step skips the misaligned weight, which is quantised on its own
    st.step()
    w8b, _ = st.weight(wm)
    _same(w8b, F.quantize_ref(w, s_ref, F.E4M3), "wrappers misaligned", "weight, next step")
    # a misaligned bias: the fp8 GEMM is declined (the caller then runs in 16 bits), never refused by the binding
    bias = torch.zeros(264, dtype=BF16)
    assert st.forward_gemm(xa, wm, _C().EPI_BIAS, _misaligned(bias)) is None
    assert st.forward_gemm(xa, wm, _C().EPI_BIAS, bias.to(DEV)) is not None


def test_zz_summary():
    """The worst error / bound per kernel, output, format and dtype, and the bit-exact comparisons' mismatch counts."""
    lines = [f"{CASES['n']} comparisons; worst |got - ref| / bound per kernel, path, format, epilogue, output and dtype:"]
    lines += [f"  {tag}: {R.WORST[tag][0]:.3f}  ({R.WORST[tag][1]})" for tag in sorted(R.WORST)]
    lines.append("bit-exact comparisons (elements that differed):")
    lines += [f"  {tag}: {EXACT[tag]}" for tag in sorted(EXACT)]
    lines.append(f"accumulator term: worst |err| / (2**-24 cond) of the dense cases (F.ACC_HW = {F.ACC_HW:g} is twice the "
                 "largest, rounded up to a power of two):")
    lines += [f"  {form}: {ACC_MEAS[form]:.1f}" for form in sorted(ACC_MEAS)]
    lines += NOTES
    print("\n" + "\n".join(lines))
    path = os.environ.get("FP8_NUMERICS_WORST_OUT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert all(v[0] <= 1.0 for v in R.WORST.values()) and all(v == 0 for v in EXACT.values())
    assert all(2.0 * v <= F.ACC_HW for v in ACC_MEAS.values()), ACC_MEAS
