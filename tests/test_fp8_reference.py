"""tests/fp8_reference.py on the CPU: the OCP codec against torch's CPU float8 casts (all 256 codes, every
bf16 and fp16 pattern that is not a NaN, an fp32 boundary set, at five scales), the kernel-structured
emulations of the quantisers and of update_scales against the references, the fp32 emulation of the fp8 GEMM
inside its bound on every case of the tables, and the mutants: each is rejected by the tables, or asserted
unrejectable with the reason. torch.float8_* appears only here, as the thing the codec is compared with.
"""
import pytest
import torch

import fp8_reference as F
import gemm_reference as R

F32, F16, BF16 = F.F32, F.F16, F.BF16
F8T = {F.E4M3: torch.float8_e4m3fn, F.E5M2: torch.float8_e5m2}
FMT_IDS = lambda f: F.FMT_NAME[f]  # noqa: E731
DT_IDS = lambda t: F.DT_NAME[t]  # noqa: E731


def _torch_q(p, fmt):
    """torch's CPU cast after the clamp, as codes."""
    return p.clamp(-F.FMT_MAX[fmt], F.FMT_MAX[fmt]).to(F8T[fmt]).view(torch.uint8)


# ----------------------------------------------------------------------------
# codec
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", F.FMTS, ids=FMT_IDS)
def test_decode_all_codes(fmt):
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    mine, ref = F.decode(codes, fmt), codes.view(F8T[fmt]).float().double()
    assert torch.equal(torch.isnan(mine), torch.isnan(ref))
    ok = ~torch.isnan(ref)
    assert torch.equal(mine[ok], ref[ok]) and torch.equal(torch.signbit(mine[ok]), torch.signbit(ref[ok]))
    assert float(F.decode(torch.tensor([F.MAX_CODE[fmt]], dtype=torch.uint8), fmt)) == F.FMT_MAX[fmt]
    assert int(torch.isnan(mine).sum()) == (2 if fmt == F.E4M3 else 6)
    # the finite codes are a fixed point of encode(decode(.))
    fin = codes[torch.isfinite(ref)]
    assert torch.equal(F.encode(F.decode(fin, fmt), fmt), fin)


@pytest.mark.parametrize("fmt", F.FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("dt", [BF16, F16], ids=DT_IDS)
def test_encode_matches_torch_on_every_16_bit_pattern(dt, fmt):
    x = F.bit_patterns(dt, finite_only=False)
    assert x.numel() == (65536 - 2 * 127 if dt == BF16 else 65536 - 2 * 1023)
    for s in F.SCALES:
        p = F.scaled(x, s)
        assert torch.equal(p, x.float() * torch.tensor(s, dtype=torch.float32))     # the fp32 product, both ways
        got, ref = F.quantize_ref(x, s, fmt), _torch_q(p, fmt)
        assert torch.equal(got, ref), (s, int((got != ref).sum()))
        # without the clamp: overflow to NaN (e4m3) / inf (e5m2), as torch's unclamped cast has it
        assert torch.equal(F.encode(p, fmt, saturate=False), p.to(F8T[fmt]).view(torch.uint8)), s


@pytest.mark.parametrize("fmt", F.FMTS, ids=FMT_IDS)
def test_encode_matches_torch_on_the_boundary_set(fmt):
    x = F.boundary_set(fmt)
    vals = F.decode(torch.arange(0, F.MAX_CODE[fmt] + 1, dtype=torch.uint8), fmt).float()
    have = set(x.tolist())
    mids = ((vals[:-1].double() + vals[1:].double()) / 2).float()
    inf = torch.tensor(float("inf"))
    for need in (vals, -vals, mids, torch.nextafter(mids, inf), torch.nextafter(mids, -inf)):
        assert set(need.tolist()) <= have
    sub = float(vals[1])
    assert {sub, sub / 2, F.FMT_MAX[fmt], -F.FMT_MAX[fmt]} <= have
    assert float(torch.nextafter(torch.tensor(F.FMT_MAX[fmt]), inf)) in have
    assert bool(((x == 0) & torch.signbit(x)).any()) and bool(((x == 0) & ~torch.signbit(x)).any())
    for s in F.SCALES:
        p = F.scaled(x, s)
        got, ref = F.quantize_ref(x, s, fmt), _torch_q(p, fmt)
        assert torch.equal(got, ref), (s, int((got != ref).sum()))
        assert torch.equal(F.encode(p, fmt, saturate=False), p.to(F8T[fmt]).view(torch.uint8)), s
        # ties go to the even code: the tie inputs of this scale are hit
    ties = F.quantize_ref(mids, 1.0, fmt)
    assert bool((ties[1:-1] % 2 == 0).all())


def test_nonfinite_reference_values():
    """What the references say about non-finite input (the GPU test pins the kernels to it)."""
    x = torch.tensor([1.0, float("nan"), float("inf"), -float("inf"), -3.0])
    for fmt in F.FMTS:
        q = F.quantize_ref(x, 1.0, fmt)
        assert q.tolist() == [int(F.encode(torch.tensor([1.0]), fmt)), F.NAN_CODE[fmt], F.MAX_CODE[fmt],
                              F.MAX_CODE[fmt] | 0x80, int(F.encode(torch.tensor([-3.0]), fmt))]
        assert F.NAN_CODE[fmt] == F.MAX_CODE[fmt] | 0x80
    assert F.amax_ref(x) == float("inf") and F.amax_ref(x[[0, 1, 4]]) == 3.0
    for a in (0.0, float("inf"), float("nan")):
        assert F.current_scale(a, 448.0) == (1.0, 1.0)


# ----------------------------------------------------------------------------
# quantiser emulations and mutants
# ----------------------------------------------------------------------------
_Q = {}


def _q_cases(scales=None):
    """(name, x, s, fmt, cur, smax) over the tables: the 16-bit patterns and the boundary set at every scale (or the
    given ones), a vector-plus-tail cut whose largest element sits in the tail, and current scaling. Built once."""
    if "cases" not in _Q:
        _Q["cases"] = list(_q_build())
    return [c for c in _Q["cases"] if scales is None or c[2] is None or c[2] in scales]


def _q_build():
    for fmt in F.FMTS:
        for dt in F.IN_DTYPES:
            tab = F.quant_table(dt, fmt)
            for s in F.SCALES:
                yield f"{F.FMT_NAME[fmt]} {F.DT_NAME[dt]} s={s:g}", tab[:tab.numel() // 8 * 8 - 3], s, fmt, None, None
        for name, x in F.amax_cases(BF16, F.QUANT_LENGTHS[:2]):
            yield f"{F.FMT_NAME[fmt]} {name}", x, 37.5, fmt, None, None
            yield f"{F.FMT_NAME[fmt]} {name} current", x, None, fmt, F.amax_ref(x), F.FMT_MAX[fmt] * 0.5


def _q_outputs(name, x, s, fmt, cur, smax, mut=None):
    return F.emu_quantize(x, s, fmt, cur, smax, mut)


def _q_expected(name, x, s, fmt, cur, smax):
    """The reference's outputs of one case, computed once."""
    if name not in _Q:
        sinv = None
        if cur is not None:
            s, sinv = F.current_scale(cur, smax)
        _Q[name] = (F.quantize_ref(x, s, fmt), F.amax_ref(x), s, sinv)
    return _Q[name]


def test_quantizer_emulation_is_the_reference():
    n = 0
    for case in _q_cases():
        codes, amax, s, sinv = _q_outputs(*case)
        rc, ra, rs, rsi = _q_expected(*case)
        assert torch.equal(codes, rc) and amax == ra and s == F.f32(rs) and sinv == rsi, case[0]
        n += 1
    assert n == 2 * (3 * 5 + 2 * 8)


@pytest.mark.parametrize("mut", F.Q_MUTANTS)
def test_quantizer_mutant_rejected(mut):
    rejected = []
    # (two of the five scales: 37.5 saturates and 2**-7 reaches the subnormals and zero; every mutant shows there)
    for case in _q_cases(scales=(37.5, 2.0 ** -7)):
        codes, amax, s, sinv = _q_outputs(*case, mut=mut)
        rc, ra, rs, rsi = _q_expected(*case)
        if not (torch.equal(codes, rc) and amax == ra and s == F.f32(rs) and sinv == rsi):
            rejected.append(case[0])
    print(f"{mut}: rejected on {len(rejected)} cases, e.g. {rejected[:3]}")
    assert rejected, mut
    if mut == "fnuz":       # (the e5m2 tables cannot see an e4m3 encoding)
        assert all(r.startswith("e4m3") for r in rejected)


def test_transposed_quantizer_and_its_mutant():
    seen = 0
    for (r, c) in F.QT_SHAPES:
        for dt in F.IN_DTYPES:
            x = (torch.randn(r, c, generator=R._gen(f"qt-{r}x{c}")) * 3).to(dt)
            for fmt in F.FMTS:
                ref = F.quantize_ref(x, 11.0, fmt).t().contiguous()
                got, amax = F.emu_quantize_t(x, 11.0, fmt)
                assert torch.equal(got, ref) and amax == F.amax_ref(x)
                bad, _ = F.emu_quantize_t(x, 11.0, fmt, mut="tile_rc_swapped")
                if r >= 64 and c >= 64:       # (the mutant lives in full 64 x 64 tiles)
                    assert not torch.equal(bad, ref), (r, c)
                    seen += 1
    assert seen == 3 * 3 * 2 and set(F.QT_MUTANTS) == {"tile_rc_swapped"}


def _run_updates(fn, hist_len, **kw):
    (hist, amax, scale, sinv, fmax), calls = F.update_scales_scenario(hist_len)
    states = []
    for a, idx, margin in calls:
        amax = amax.clone()
        amax[:] = a
        hist, amax, scale, sinv = fn(hist, amax, scale, sinv, fmax, F.US_N, idx, margin, **kw)
        states.append((hist, amax, scale, sinv))
    return states


def _same_states(a, b):
    return all(torch.equal(x.nan_to_num(nan=-1.0), y.nan_to_num(nan=-1.0)) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


@pytest.mark.parametrize("hist_len", [1, 16])
def test_update_scales_emulation_is_the_reference(hist_len):
    ref = _run_updates(F.update_scales_ref, hist_len)
    assert _same_states(_run_updates(F.emu_update_scales, hist_len), ref)
    (hist0, _, scale0, sinv0, fmax), calls = F.update_scales_scenario(hist_len)
    hist, amax, scale, sinv = ref[-1]
    z = F.US_ZERO_SLOT
    assert float(scale[z]) == float(scale0[z]) and float(sinv[z]) == float(sinv0[z])          # all-zero window
    assert torch.equal(scale[F.US_N:], scale0[F.US_N:]) and torch.equal(hist[F.US_N:], hist0[F.US_N:])
    assert bool((amax[:F.US_N] == 0).all()) and bool((amax[F.US_N:] == calls[-1][0][F.US_N:]).all())
    assert bool(torch.isfinite(hist).all()) and bool(torch.isfinite(scale).all())               # inf / NaN recorded as 0
    # one slot by hand: the last call's margin on the window's max, in the kernel's operation order
    a = hist[0].max()
    assert float(scale[0]) == float((fmax[0] / a) * torch.tensor(F.US_MARGINS[2]))
    assert float(sinv[0]) == float(1.0 / scale[0])


@pytest.mark.parametrize("mut", F.US_MUTANTS)
def test_update_scales_mutant_rejected(mut):
    ref = _run_updates(F.update_scales_ref, 16)
    assert not _same_states(_run_updates(F.emu_update_scales, 16, mut=mut), ref), mut
    if mut != "hist_max_short":     # (a window of one entry has no shorter max)
        assert not _same_states(_run_updates(F.emu_update_scales, 1, mut=mut), _run_updates(F.update_scales_ref, 1)), mut


# ----------------------------------------------------------------------------
# fp8 GEMM: emulation inside the bound, integer cases, mutants
# ----------------------------------------------------------------------------
def _bdts(epi, T):
    return (F32, T) if R.colsum(epi) else (None,)


_ACC = {}


def _case(shape, fa, T):
    """Operands and the float64 product of one (shape, format) — computed once and shared, left unchanged."""
    key = (shape.name, fa, T)
    if key not in _ACC:
        ops = F.dense_operands(shape.name, shape.M, shape.N, shape.K, fa, T)
        other = _ACC.get((shape.name, fa, BF16 if T == F16 else F16))
        _ACC[key] = (ops, other[1] if other else F.acc_ref(ops[0], ops[1], fa, F.E4M3, F.alpha_of(ops[2], ops[3])))
    return _ACC[key]


def _emu_ratio(shape, fa, T, epi, bdt, mut=None, worst=None, tag=None):
    (A8, B8, aa, ab, bias, aux), (acc, cond) = _case(shape, fa, T)
    c, x = F.emu_gemm(epi, T, A8, B8, fa, aa, ab, bias, aux, bdt, mut)
    return F.check_epilogue(epi, T, shape.K, acc, cond, c, x, bias, aux, bdt,
                            what=f"{shape.name} {F.FMT_NAME[fa]} {F.DT_NAME[T]}", tag=tag, worst=worst)


@pytest.mark.parametrize("fa", F.FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("shape", F.NT_SHAPES, ids=[s.name for s in F.NT_SHAPES])
def test_gemm_emulation_within_bound(shape, fa):
    for T in R.DTYPES:
        for epi in R.EPIS:
            for bdt in _bdts(epi, T):
                r = _emu_ratio(shape, fa, T, epi, bdt, tag="emu f8")
                print(f"{shape.name} {F.FMT_NAME[fa]} {F.DT_NAME[T]} {epi} db={F.DT_NAME[bdt]}: worst error / bound {r:.3f}")


def test_dense_codes_cover_the_format_range():
    for fmt in F.FMTS:
        c = F.dense_codes("cover", 256, 384, fmt)
        mag = c & 0x7f
        assert int(mag.max()) == F.MAX_CODE[fmt] and bool((mag < (1 << F.MBITS[fmt])).any())      # max; subnormals
        assert bool(torch.isfinite(F.decode(c, fmt)).all())
        assert len(torch.unique(c)) > (200 if fmt == F.E4M3 else 150)
    for fa in F.FMTS:
        aa, ab = F.dense_alphas(256, fa)
        assert all(torch.frexp(torch.tensor(v))[0] != 0.5 for v in (aa, ab, F.alpha_of(aa, ab)))   # no power of two


@pytest.mark.parametrize("fa", F.FMTS, ids=FMT_IDS)
def test_exact_cases_are_exact_in_the_emulation(fa):
    for shape in F.NT_SHAPES:
        A8, B8, A, B, bias, aux = F.exact_operands(shape.M, shape.N, shape.K, fa)
        assert F.alpha_of(*F.EXACT_ALPHA) == 1.0 and F.EXACT_ALPHA[0] != 1.0
        for T in R.DTYPES:
            for epi in R.EXACT_EPIS:
                c, x = F.emu_gemm(epi, T, A8, B8, fa, *F.EXACT_ALPHA, bias.to(T), aux.to(T), F32 if epi == "mul" else None)
                for name, v in R.exact_expected(epi, A, B, bias, aux).items():
                    assert torch.equal((c if name == "C" else x).double(), v.double()), (shape.name, epi, name)
                # a dropped alpha_b doubles every integer
                c2, _ = F.emu_gemm("none", T, A8, B8, fa, *F.EXACT_ALPHA, mut="alpha_a_only")
                assert torch.equal(c2.double(), 2 * R.exact_acc(A, B).double())


@pytest.mark.parametrize("mut", sorted(F.GEMM_MUTANTS))
def test_gemm_mutant_rejected(mut):
    """Outside the bound on at least one case of its class, while the correct emulation is inside on all of them."""
    rejected, seen = [], 0
    for shape in (F.NT_FULL[1], F.NT_EDGE[1], F.NT_EDGE[3]):     # (a small shape of each class is enough, and quick)
        for fa in F.FMTS:
            for T in R.DTYPES:
                for epi in ("none", "bias_gelu_d", "mul"):
                    if not F.GEMM_MUTANTS[mut](epi, fa):
                        continue
                    bdt = F32 if R.colsum(epi) else None
                    assert _emu_ratio(shape, fa, T, epi, bdt, worst={}) <= 1.0
                    bad = _emu_ratio(shape, fa, T, epi, bdt, mut=mut, worst={})
                    seen += 1
                    if bad > 1.0:
                        rejected.append((shape.name, F.FMT_NAME[fa], F.DT_NAME[T], epi, round(bad, 2)))
    print(f"{mut}: rejected on {len(rejected)} of {seen} cases, e.g. {rejected[:3]}")
    assert seen and rejected, mut
    if mut not in ("alpha_after_rounding", "erf_tanh_swap"):    # (those are wrong on some elements, not on every shape)
        assert len(rejected) == seen, (mut, len(rejected), seen)


def test_alpha_fl32_rounding_is_not_rejectable():
    """alpha kept in float64 (alpha_a * alpha_b never rounded to fp32) only removes a rounding: the bound has to
    admit the correct kernel, which rounds, and an implementation that is closer to the float64 reference than
    the correct one cannot be outside a bound that is centred on that reference's own alpha up to 2**-24 |acc*|
    — half of the `stage` term. Asserted unrejectable: its distance from the reference is inside the bound."""
    shape, fa, T = F.NT_SHAPES[0], F.E5M2, BF16
    (A8, B8, aa, ab, bias, aux), (acc, cond) = _case(shape, fa, T)
    exact_alpha = float(aa) * float(ab)
    acc64 = acc / F.alpha_of(aa, ab) * exact_alpha
    c = acc64.float().to(T)
    assert R.ratio(c, *R.expected("none", T, shape.K, acc, cond, stage=F.E24)["C"])[0] <= 1.0


@pytest.mark.parametrize("q8_fmt", F.FMTS, ids=FMT_IDS)
def test_q8_reference_and_mutant(q8_fmt):
    """Codes of the stored (rounded) C; a mutant that encodes the unrounded fp32 value is told apart."""
    shape, fa, T = F.Q8_SHAPES[1], F.E4M3, BF16
    (A8, B8, aa, ab, bias, aux), _ = _case(shape, fa, T)
    c, _ = F.emu_gemm("mul", T, A8, B8, fa, aa, ab, bias, aux, None)
    a, b = F.decode(A8, fa).float(), F.decode(B8, F.E4M3).float()
    unrounded = R._rnd((a @ b.t()) * torch.tensor(F.alpha_of(aa, ab)), T) * aux.float()
    scale = F.f32(0.37 * F.FMT_MAX[q8_fmt] / F.amax_ref(c))
    codes, amax = F.q8_expected(c, scale, q8_fmt, prev_amax=0.5)
    assert torch.equal(F.emu_q8(c, unrounded, scale, q8_fmt), codes) and amax == float(c.float().abs().max())
    assert F.q8_expected(c, scale, q8_fmt, prev_amax=1e9)[1] == 1e9
    assert not torch.equal(F.emu_q8(c, unrounded, scale, q8_fmt, mut="q8_from_unrounded"), codes)


@pytest.mark.parametrize("fa", F.FMTS, ids=FMT_IDS)
def test_wgrad_emulation_exact_cases_and_mutants(fa):
    for (Rr, P, Q, s) in F.WGRAD:
        A8, B8, aa, ab = F.dense_wgrad_operands(f"{Rr}x{P}x{Q}", Rr, P, Q, fa)
        alpha = F.alpha_of(aa, ab)
        for odt in (F32, BF16, F16):
            ref, bound = F.wgrad_expected(A8, B8, fa, F.E4M3, alpha, s, odt)
            r = R.check(F.emu_wgrad(A8, B8, fa, F.E4M3, alpha, s, odt), ref, bound, f"wgrad f8 {Rr}x{P}x{Q} s{s}",
                        f"emu f8 wgrad {F.FMT_NAME[fa]}->{F.DT_NAME[odt]}")
            assert r <= 1.0
        # mutants: alpha_a alone; the operand formats swapped / e5m2 read as e4m3
        ref, bound = F.wgrad_expected(A8, B8, fa, F.E4M3, alpha, s, F32)
        assert R.ratio(F.emu_wgrad(A8, B8, fa, F.E4M3, F.f32(aa), s, F32), ref, bound)[0] > 1.0
        if fa == F.E5M2:
            assert R.ratio(F.emu_wgrad(A8, B8, F.E4M3, F.E4M3, alpha, s, F32), ref, bound)[0] > 1.0
            assert R.ratio(F.emu_wgrad(A8, B8, F.E4M3, fa, alpha, s, F32), ref, bound)[0] > 1.0
        # integer case: bit-exact in fp32
        E8, G8, A, B, _, _ = F.exact_operands(P, Q, Rr, fa)
        got = F.emu_wgrad(E8.t().contiguous(), G8.t().contiguous(), fa, F.E4M3, F.alpha_of(*F.EXACT_ALPHA), s, F32)
        assert torch.equal(got.double(), R.exact_acc(A, B).double())
    assert F.wgrad_slices(384, 2) == [(0, 1), (1, 3)] and F.wgrad_slices(384, 3) == [(0, 1), (1, 2), (2, 3)]


def test_case_tables():
    """The cases the GPU file is asked to run are in the tables."""
    assert [(s.M, s.N, s.K) for s in F.NT_FULL] == [(256, 256, k) for k in (128, 256, 384)]
    assert {(s.M, s.N, s.K) for s in F.NT_EDGE} == {(1, 8, 128), (8, 8, 128), (300, 392, 384), (257, 264, 256)}
    assert {s.layout for s in F.NT_LAYOUT} == {"lda", "a3d"}
    assert F.WGRAD == [(128, 256, 256, 1), (384, 256, 256, 2), (384, 256, 256, 3), (256, 16, 272, 1), (256, 272, 16, 1),
                       (640, 528, 272, 2)]
    assert F.QT_SHAPES == [(1, 1), (7, 9), (8, 64), (64, 8), (64, 64), (65, 63), (130, 72), (300, 200)]
    assert F.QUANT_LENGTHS == [3, 8 * 256 + 5, 2 ** 21 + 8 * 256 + 3] and F.SCALES == [1.0, 37.5, 2.0 ** -7, 1e4, 3e38]
    for cus in (256, 304, 64):
        s = F.persist_shape(cus, 128)
        assert (s.M // 256) * (s.N // 256) > cus and s.M % 256 == 0 and s.K % 128 == 0
    rc = [(r, c) for r, c, _ in F.WQ_WEIGHTS]
    assert any(c % 8 for _, c in rc) and any(r % 8 for r, _ in rc) and any(r * c % 8 for r, c in rc)
    assert any(r * c > 65536 for r, c in rc) and (1, 1) in rc and {t for _, _, t in F.WQ_WEIGHTS} == {True, False}
    assert sorted(F.WQ_SLOTS) != F.WQ_SLOTS and len(set(F.WQ_SLOTS)) == len(F.WQ_WEIGHTS) < F.WQ_NSLOTS
    assert len(R.EPIS) == 10 and len(F.Q8_EPIS) == 7


def test_zz_summary():
    print("\nworst |emulation - ref| / bound per output and dtype:")
    for tag in sorted(t for t in R.WORST if t.startswith("emu f8")):
        print(f"  {tag}: {R.WORST[tag][0]:.3f}  ({R.WORST[tag][1]})")
    assert all(v[0] <= 1.0 for t, v in R.WORST.items() if t.startswith("emu f8"))
