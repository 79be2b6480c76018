"""Float64 reference of the multi-tensor ops (csrc/multi_tensor.hip) and the shared test cases.

A plain helper module: no tests, no fixtures. It holds

* straight float64 PyTorch-on-CPU implementations of scale, axpby, l2norm, SGD, Adam/AdamW, LAMB
  and LARC, written from the formulas in the kernel header comments and apex/parallel/LARC.py.
  They never call apex.multi_tensor_apply.ops. Gradients enter at their stored (16-bit or fp32)
  values converted to double; every other quantity is double;
* the size sets, optimizer cases and input generators that tests/test_mt_reference.py (fp32 CPU
  path against this reference) and tests/test_multi_tensor_gpu.py (HIP kernels against this
  reference) share, so both look at the same numbers;
* BOUNDS: the measured error of the fp32 CPU path against this reference for every case. The GPU
  tests allow MARGIN times these.

Hyper-parameters: the kernels take them as fp32. A value such as 0.999 is not an fp32 number, and
`1.f - 0.999f` is 1.3e-5 away (relative) from 0.001, which is far above fp32 rounding of the
state. That is a property of an fp32 interface, not of the arithmetic under test, so every case
rounds its hyper-parameters to fp32 once (f32 below) and gives the same values to the reference,
to the fp32 CPU path and to the kernels.
"""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass, field

import torch

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
DT_NAME = {F32: "f32", F16: "f16", BF16: "bf16", None: "none"}

# half an ulp relative to the value: the worst error of one correct rounding to that dtype
HALF_ULP = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}
# smallest positive spacing (subnormal step) of the dtype
TINY = {F32: 2.0 ** -149, F16: 2.0 ** -24, BF16: 2.0 ** -133}

MARGIN = 4.0        # GPU tests allow MARGIN * BOUNDS[case]
NORM_RTOL = 1e-4    # norms against fp64: <= 128 sequential fp32 adds per lane ~ 8e-6, tenfold margin

DEFAULT_CHUNK = 32768
SMALL_CHUNK = 64
# structural edges of stream_for (4096 steps, 1024 strides, scalar tail) and of the chunk table
SIZES_DEFAULT = [0, 1, 3, 4, 5, 1023, 1027, 4095, 4096, 4099, 5123, 32768, 32769, 36867, 65541]
# with chunk_size 64: 2052 chunks in the first tensor, so the grid-stride loop (2048 blocks) wraps
SIZES_MANY = [64 * 2051 + 5, 1, 63, 64, 65, 200]
# chunk_for edges (8-element groups, 2048-element sweep)
SIZES_AXPBY_EDGES = [7, 8, 9, 2047, 2048, 2055]
SIZE_SETS = {"default": (SIZES_DEFAULT, DEFAULT_CHUNK), "many": (SIZES_MANY, SMALL_CHUNK)}
MIXED_UNALIGNED_INDEX = 5   # "mixed" placement: only this tensor is off 16-byte alignment
# LAMB cases: one all-zero parameter tensor and one all-zero gradient tensor (index into either set)
LAMB_ZERO_PARAM = {"default": 6, "many": 2}
LAMB_ZERO_GRAD = {"default": 9, "many": 4}
NSTEPS = 3


def f32(x: float) -> float:
    """x rounded to fp32, as a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float32))


# ----------------------------------------------------------------------------
# float64 reference implementations
# ----------------------------------------------------------------------------
def ref_scale(xs, s):
    """out = in * s"""
    return [x.double() * float(s) for x in xs]


def ref_axpby(xs, ys, a, b):
    """out = a*x + b*y"""
    return [float(a) * x.double() + float(b) * y.double() for x, y in zip(xs, ys)]


def ref_nonfinite(xs) -> bool:
    return any(not bool(torch.isfinite(x.double()).all()) for x in xs)


def ref_l2norm(xs, s=1.0):
    """(global norm, [per-tensor norms]): sqrt(sum x^2) * s"""
    sq = [float((x.double() ** 2).sum()) for x in xs]
    return math.sqrt(sum(sq)) * float(s), [math.sqrt(v) * float(s) for v in sq]


def ref_sgd_step(gs, ps, moms, *, lr, momentum, dampening, wd, nesterov, first_run,
                 wd_after_momentum, scale=1.0):
    """In place on the double lists ps, moms.
    g' = g*scale (+ wd*p before momentum); buf = g' on the first run, else
    momentum*buf + (1-dampening)*g'; d = g' + momentum*buf (nesterov) or buf;
    (+ wd*p after momentum); p -= lr*d."""
    for g, p, buf in zip(gs, ps, moms):
        d = g.double() * scale
        if wd != 0 and not wd_after_momentum:
            d = d + wd * p
        if momentum != 0:
            if first_run:
                buf.copy_(d)
            else:
                buf.copy_(momentum * buf + (1.0 - dampening) * d)
            d = d + momentum * buf if nesterov else buf.clone()
        if wd != 0 and wd_after_momentum:
            d = d + wd * p
        p.sub_(lr * d)


def ref_adam_step(gs, ps, ms, vs, *, lr, beta1, beta2, eps, step, adamw, bias_correction, wd,
                  grad_scale=1.0):
    """In place on the double lists ps, ms, vs.
    g' = g*scale (+ wd*p in L2 mode); m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2;
    u = (m/bc1) / (sqrt(v/bc2) + eps) (+ wd*p in AdamW mode); p -= lr*u."""
    bc1 = 1.0 - beta1 ** step if bias_correction else 1.0
    bc2 = 1.0 - beta2 ** step if bias_correction else 1.0
    for g, p, m, v in zip(gs, ps, ms, vs):
        d = g.double() * grad_scale
        if not adamw and wd != 0:
            d = d + wd * p
        m.copy_(beta1 * m + (1.0 - beta1) * d)
        v.copy_(beta2 * v + (1.0 - beta2) * d * d)
        u = (m / bc1) / ((v / bc2).sqrt() + eps)
        if adamw and wd != 0:
            u = u + wd * p
        p.sub_(lr * u)


def ref_lamb_step(gs, ps, ms, vs, *, lr, beta1, beta2, eps, step, bias_correction, wd,
                  grad_averaging, adamw, max_grad_norm, use_nvlamb, grad_scale=1.0, gnorm=None):
    """In place on the double lists ps, ms, vs; returns the global gradient norm it used.
    norm = ||g||*scale over all tensors unless supplied; clip = norm/max when max > 0 and
    norm > max, else 1; g' = g*scale/clip (+ wd*p in L2 mode); m = b1 m + b3 g' with
    b3 = 1-b1 (grad_averaging) or 1; v = b2 v + (1-b2) g'^2;
    u = (m/bc1)/(sqrt(v/bc2)+eps) (+ wd*p in AdamW mode);
    p -= lr * r * u, r = ||p||/||u|| per tensor when (wd != 0 or use_nvlamb) and both norms
    are non-zero, else 1."""
    if gnorm is None:
        gnorm = ref_l2norm(gs, grad_scale)[0]
    gnorm = float(gnorm)
    clip = gnorm / max_grad_norm if (max_grad_norm > 0 and gnorm > max_grad_norm) else 1.0
    bc1 = 1.0 - beta1 ** step if bias_correction else 1.0
    bc2 = 1.0 - beta2 ** step if bias_correction else 1.0
    b3 = 1.0 - beta1 if grad_averaging else 1.0
    for g, p, m, v in zip(gs, ps, ms, vs):
        d = g.double() * grad_scale / clip
        if not adamw and wd != 0:
            d = d + wd * p
        m.copy_(beta1 * m + b3 * d)
        v.copy_(beta2 * v + (1.0 - beta2) * d * d)
        u = (m / bc1) / ((v / bc2).sqrt() + eps)
        if adamw and wd != 0:
            u = u + wd * p
        r = 1.0
        if use_nvlamb or wd != 0:
            pn, un = math.sqrt(float((p * p).sum())), math.sqrt(float((u * u).sum()))
            if pn != 0 and un != 0:
                r = pn / un
        p.sub_(lr * r * u)
    return gnorm


def ref_larc_grads(gs, ps, *, trust, eps, lr, wd, clip):
    """The gradients LARC hands to the wrapped optimizer (double).
    a = trust*||p|| / (||g|| + wd*||p|| + eps); clip mode: a = min(a/lr, 1);
    g' = (g + wd*p) * a; g untouched when either norm is zero."""
    out = []
    for g, p in zip(gs, ps):
        gd, pd = g.double(), p.double()
        pn, gn = math.sqrt(float((pd * pd).sum())), math.sqrt(float((gd * gd).sum()))
        if pn == 0 or gn == 0:
            out.append(gd.clone())
            continue
        a = trust * pn / (gn + pn * wd + eps)
        if clip:
            a = min(a / lr, 1.0)
        out.append((gd + wd * pd) * a)
    return out


# ----------------------------------------------------------------------------
# comparison helpers
# ----------------------------------------------------------------------------
def max_abs_err(got, ref) -> float:
    """Largest |got - ref| over two parallel lists (got in any dtype, ref double)."""
    worst = 0.0
    for a, b in zip(got, ref):
        assert a.shape == b.shape, (a.shape, b.shape)
        if a.numel():
            d = (a.detach().cpu().double() - b).abs()
            assert bool(torch.isfinite(d).all()), "non-finite value in result"
            worst = max(worst, float(d.max()))
    return worst


def ulp_excess(got, ref, dtype, extra=None) -> float:
    """max over elements of |got - ref| / tol, tol = HALF_ULP*|ref| + subnormal step (+ extra):
    <= 1 when got is ref rounded once to dtype (extra: error of the fp32 evaluation before it)."""
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, ref)):
        if not a.numel():
            continue
        tol = HALF_ULP[dtype] * b.abs() + TINY[dtype]
        if extra is not None:
            tol = tol + extra[i]
        worst = max(worst, float(((a.detach().cpu().double() - b).abs() / tol).max()))
    return worst


# ----------------------------------------------------------------------------
# shared inputs
# ----------------------------------------------------------------------------
def randn_list(sizes, seed, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).to(dtype) for n in sizes]


@dataclass(frozen=True)
class Case:
    op: str            # "sgd" | "adam" | "lamb"
    name: str
    sizes: str         # key of SIZE_SETS
    gdt: torch.dtype   # gradient dtype
    cdt: object        # dtype of the 16-bit copy list, or None
    scale: float       # gradient scale (1.0: none)
    hp: tuple = field(default=())   # op-specific hyper-parameters, as (name, value) pairs

    @property
    def key(self):
        return f"{self.op}/{self.name}"

    @property
    def h(self):
        return dict(self.hp)

    @property
    def chunk(self):
        return SIZE_SETS[self.sizes][1]

    @property
    def sizelist(self):
        return SIZE_SETS[self.sizes][0]


def _case(op, name, sizes, gdt, cdt, scale, **hp):
    hp = tuple((k, f32(v) if isinstance(v, float) else v) for k, v in hp.items())
    return Case(op, name, sizes, gdt, cdt, f32(scale), hp)


def _sgd(name, sizes, gdt, cdt, scale, momentum, nesterov, dampening, wd, after):
    return _case("sgd", name, sizes, gdt, cdt, scale, lr=1e-2, momentum=float(momentum),
                 nesterov=nesterov, dampening=float(dampening), wd=float(wd),
                 wd_after_momentum=after)


# a covering set: momentum {0, .9} x nesterov x dampening {0, .1} x wd placement x gradient
# dtype/scale x copy dtype x size set
SGD_CASES = [
    _sgd("plain-f32", "default", F32, None, 1.0, 0.0, False, 0.0, 0.0, False),
    _sgd("plain-wd-bf16-cbf16", "default", BF16, BF16, 0.5, 0.0, False, 0.0, 0.1, False),
    _sgd("plain-wdafter-f32", "default", F32, None, 1.0, 0.0, False, 0.0, 0.1, True),
    _sgd("nest-wd-f32", "default", F32, None, 1.0, 0.9, True, 0.0, 0.1, False),
    _sgd("nest-wdafter-bf16-cbf16", "default", BF16, BF16, 0.5, 0.9, True, 0.0, 0.1, True),
    _sgd("mom-wd-f16-cf16", "default", F16, F16, 1.0 / 128, 0.9, False, 0.0, 0.1, False),
    _sgd("mom-damp-wd-f32", "default", F32, None, 1.0, 0.9, False, 0.1, 0.1, False),
    _sgd("mom-damp-wdafter-f16", "default", F16, None, 1.0 / 128, 0.9, False, 0.1, 0.1, True),
    _sgd("mom-f32-cbf16", "default", F32, BF16, 1.0, 0.9, False, 0.0, 0.0, False),
    _sgd("mom-damp-wdafter-bf16-cbf16-many", "many", BF16, BF16, 0.5, 0.9, False, 0.1, 0.1, True),
    _sgd("nest-wd-f32-cf16-many", "many", F32, F16, 1.0, 0.9, True, 0.0, 0.1, False),
    _sgd("plain-wd-f16-many", "many", F16, None, 1.0 / 128, 0.0, False, 0.0, 0.1, False),
]


def _adam(name, sizes, gdt, cdt, scale, adamw, wd=0.01, bias_correction=True):
    return _case("adam", name, sizes, gdt, cdt, scale, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8,
                 wd=float(wd), adamw=adamw, bias_correction=bias_correction)


# the combined factor of the "Adam clip under amp" test: amp inverse loss scale 1/64, legacy
# scale 2, norm 10 and max_grad_norm 1 -> clip (10/2 + 1e-6)/1
ADAM_CLIP_AMP = dict(amp_scale=1.0 / 64, scale=2.0, norm=10.0, max_grad_norm=1.0)
ADAM_CLIP_FACTOR = ADAM_CLIP_AMP["amp_scale"] * f32((1.0 / ADAM_CLIP_AMP["scale"]) / (
    (ADAM_CLIP_AMP["norm"] / ADAM_CLIP_AMP["scale"] + 1e-6) / ADAM_CLIP_AMP["max_grad_norm"]))

ADAM_CASES = [
    _adam("adamw-f32", "default", F32, None, 1.0, True),
    _adam("adamw-bf16-cbf16", "default", BF16, BF16, 1.0 / 128, True),
    _adam("l2-f32", "default", F32, None, 1.0, False),
    _adam("l2-bf16-cbf16", "default", BF16, BF16, 1.0 / 128, False),
    _adam("l2-f32-cf16-nobc", "default", F32, F16, 0.5, False, bias_correction=False),
    _adam("adamw-bf16-cbf16-many", "many", BF16, BF16, 1.0 / 128, True),
    _adam("l2-f32-many", "many", F32, None, 1.0, False),
    _adam("adamw-f32-clipamp", "default", F32, None, ADAM_CLIP_FACTOR, True),
]


def _lamb(name, sizes, gdt, cdt, scale, wd, nvlamb, ga, adamw, mgn, supplied):
    return _case("lamb", name, sizes, gdt, cdt, scale, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-6,
                 wd=float(wd), use_nvlamb=nvlamb, grad_averaging=ga, adamw=adamw,
                 max_grad_norm=float(mgn), supplied_norm=supplied, bias_correction=True)


# "bench": bf16 gradients, fp32 masters, bf16 copies, device gradient scale (amp O2 fused master).
# max_grad_norm 1.0 is far below every case's gradient norm, so the clip is active where set.
LAMB_CASES = [
    _lamb("bench-wd-adamw-clip", "default", BF16, BF16, 1.0 / 128, 0.01, False, True, True, 1.0, False),
    _lamb("f32-wd0-adamw-noclip", "default", F32, None, 1.0, 0.0, False, True, True, 0.0, False),
    _lamb("f32-wd0-nvlamb-l2-clip-gnorm", "default", F32, None, 1.0, 0.0, True, False, False, 1.0, True),
    _lamb("f32-wd-l2-noavg-noclip", "default", F32, None, 1.0, 0.01, False, False, False, 0.0, False),
    _lamb("bench-wd-l2-noavg-gnorm-many", "many", BF16, BF16, 1.0 / 128, 0.01, False, False, False, 0.0, True),
    _lamb("f32-wd-adamw-nvlamb-clip-many", "many", F32, None, 1.0, 0.01, True, True, True, 1.0, False),
]

LARC_CASES = [(clip, wd) for clip in (True, False) for wd in (0.0, f32(5e-4))]
LARC_HP = dict(trust=f32(0.02), eps=f32(1e-8), lr=f32(0.1))
LARC_SIZES = [5, 1027, 4099, 36867, 2055, 8]   # one multi-chunk tensor
LARC_ZERO_GRAD, LARC_ZERO_PARAM = 1, 4

CASES = {c.key: c for c in SGD_CASES + ADAM_CASES + LAMB_CASES}


def case_inputs(case: Case):
    """(params fp32, [gradients of step k in case.gdt]) on the CPU; fresh tensors on every call."""
    seed = zlib.crc32(case.key.encode()) & 0x7FFFFFFF
    ps = randn_list(case.sizelist, seed)
    grads = [randn_list(case.sizelist, seed + 1 + k, case.gdt) for k in range(NSTEPS)]
    if case.op == "lamb":
        ps[LAMB_ZERO_PARAM[case.sizes]].zero_()
        for gk in grads:
            gk[LAMB_ZERO_GRAD[case.sizes]].zero_()
    return ps, grads


def lamb_supplied_norm(case: Case, grads_k) -> float:
    """The norm handed to the op in the supplied-norm cases: 1.25 x the true one, rounded to fp32,
    so an op that ignored it and used its own would be caught."""
    return f32(1.25 * ref_l2norm(grads_k, case.scale)[0])


@functools.lru_cache(maxsize=None)
def reference(key: str, nsteps: int = NSTEPS):
    """Float64 state after nsteps of case `key`: {"p", "m", "v", "norm"}. Computed once per
    process; callers must not modify it. SGD: "m" is the momentum buffer, "v" is empty."""
    case = CASES[key]
    h = case.h
    ps, grads = case_inputs(case)
    p = [t.double() for t in ps]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    norm = None
    for k in range(nsteps):
        if case.op == "sgd":
            ref_sgd_step(grads[k], p, m, lr=h["lr"], momentum=h["momentum"], dampening=h["dampening"],
                         wd=h["wd"], nesterov=h["nesterov"], first_run=(k == 0),
                         wd_after_momentum=h["wd_after_momentum"], scale=case.scale)
        elif case.op == "adam":
            ref_adam_step(grads[k], p, m, v, lr=h["lr"], beta1=h["beta1"], beta2=h["beta2"],
                          eps=h["eps"], step=k + 1, adamw=h["adamw"],
                          bias_correction=h["bias_correction"], wd=h["wd"], grad_scale=case.scale)
        else:
            gn = lamb_supplied_norm(case, grads[k]) if h["supplied_norm"] else None
            norm = ref_lamb_step(grads[k], p, m, v, lr=h["lr"], beta1=h["beta1"], beta2=h["beta2"],
                                 eps=h["eps"], step=k + 1, bias_correction=h["bias_correction"],
                                 wd=h["wd"], grad_averaging=h["grad_averaging"], adamw=h["adamw"],
                                 max_grad_norm=h["max_grad_norm"], use_nvlamb=h["use_nvlamb"],
                                 grad_scale=case.scale, gnorm=gn)
    return {"p": p, "m": m, "v": [] if case.op == "sgd" else v, "norm": norm}


def larc_inputs(gdt, pdt, seed=77):
    ps = randn_list(LARC_SIZES, seed, pdt)
    gs = randn_list(LARC_SIZES, seed + 1, gdt)
    gs[LARC_ZERO_GRAD].zero_()
    ps[LARC_ZERO_PARAM].zero_()
    return gs, ps


# ----------------------------------------------------------------------------
# running a case through the project's code: apex.multi_tensor_apply.ops on `device`
# (CPU tensors: its fp32 PyTorch branch; device tensors: the HIP kernels)
# ----------------------------------------------------------------------------
def put(ts, device, place="aligned"):
    """Fresh copies of the CPU tensors `ts` on `device`. place "unaligned": every tensor is the
    view buf[1:1+n] of its own buffer (4 bytes off for fp32, 2 for 16-bit); "mixed": only tensor
    MIXED_UNALIGNED_INDEX is."""
    out = []
    for i, t in enumerate(ts):
        n = t.numel()
        if place == "unaligned" or (place == "mixed" and i == MIXED_UNALIGNED_INDEX):
            v = torch.empty(n + 1, dtype=t.dtype, device=device)[1:1 + n]
        else:
            assert place in ("aligned", "mixed"), place
            v = torch.empty(n, dtype=t.dtype, device=device)
        out.append(v.copy_(t))
    return out


def setup_case(case: Case, dev, place="aligned"):
    """(CPU gradients per step, g, p, m, v, copy or None, the op's tensor lists) on `dev`: g holds
    step 0's gradients, m and v are zero. SGD's lists are [g, p, m, (copy)]."""
    ps_c, grads_c = case_inputs(case)
    zeros = [torch.zeros_like(t) for t in ps_c]
    g = put(grads_c[0], dev, place)
    p, m, v = put(ps_c, dev, place), put(zeros, dev, place), put(zeros, dev, place)
    cp = put([z.to(case.cdt) for z in zeros], dev, place) if case.cdt is not None else None
    lists = ([g, p, m] if case.op == "sgd" else [g, p, m, v]) + ([cp] if cp is not None else [])
    return grads_c, g, p, m, v, cp, lists


def run_case(case: Case, device, *, place="aligned", scale_tensor=False, nsteps=NSTEPS):
    """NSTEPS steps of `case` through apex.multi_tensor_apply.ops (LAMB: lamb_reference on the CPU,
    the plan's lamb on the device). Returns {"p", "m", "v", "copy", "norm", "lists"}."""
    from apex.multi_tensor_apply import get_plan, ops

    h = case.h
    dev = torch.device(device)
    grads_c, g, p, m, v, cp, lists = setup_case(case, dev, place)
    sc = torch.tensor([case.scale], dtype=F32, device=dev) if scale_tensor else case.scale
    step_t = torch.zeros(1, dtype=torch.int32, device=dev)
    norm = None
    for k in range(nsteps):
        for dst, src in zip(g, grads_c[k]):
            dst.copy_(src)
        if case.op == "sgd":
            ops.multi_tensor_sgd(case.chunk, None, lists, h["wd"], h["momentum"], h["dampening"],
                                 h["lr"], h["nesterov"], k == 0, h["wd_after_momentum"], sc)
        elif case.op == "adam":
            ops.multi_tensor_adam(case.chunk, None, lists, h["lr"], h["beta1"], h["beta2"], h["eps"],
                                  k + 1, int(h["adamw"]), h["bias_correction"], h["wd"], sc)
        elif dev.type == "cpu":
            # the gradient norm as FusedLAMB's CPU branch takes it
            gn = lamb_supplied_norm(case, grads_c[k]) if h["supplied_norm"] else float(
                torch.stack([t.float().norm() for t in g]).pow(2).sum().sqrt() * case.scale)
            ops.lamb_reference(g, p, m, v, h["lr"], h["beta1"], h["beta2"], h["eps"], k + 1,
                               h["bias_correction"], h["wd"], h["grad_averaging"], int(h["adamw"]),
                               gn, h["max_grad_norm"], h["use_nvlamb"], grad_scale=case.scale,
                               copies=cp)
            norm = gn
        else:
            gn = torch.tensor([lamb_supplied_norm(case, grads_c[k])], dtype=F32, device=dev) \
                if h["supplied_norm"] else None
            ws = get_plan(lists, case.chunk).lamb(
                h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], h["max_grad_norm"], h["adamw"],
                h["bias_correction"], h["grad_averaging"], h["use_nvlamb"],
                1.0 if scale_tensor else case.scale, sc if scale_tensor else None, None, None,
                step_t, gn)
            norm = float(ws[0])
    return {"p": p, "m": m, "v": [] if case.op == "sgd" else v, "copy": cp, "norm": norm,
            "lists": lists}


def state_errors(got, ref):
    """(p, m, v) largest absolute errors of run_case's result against reference()'s."""
    return tuple(max_abs_err(got[k], ref[k]) for k in ("p", "m", "v"))


# ----------------------------------------------------------------------------
# Measured bounds: largest |fp32 CPU path - float64 reference| over all elements after the
# NSTEPS steps of each case, as (p, m or momentum buffer, v); the fp32 CPU path is
# apex.multi_tensor_apply.ops on CPU tensors (lamb_reference for LAMB, apex.parallel.LARC's CPU
# branch for LARC). Each entry is the measured figure itself, rounded up in the third digit, with
# no padding: tests/test_mt_reference.py measures again and asserts
# measured <= bound <= 1.02 * measured for every entry, so they cannot drift and the padding
# is the rounding alone (at most 1 %). The GPU tests allow MARGIN x these.
# ----------------------------------------------------------------------------
BOUNDS = {
    "sgd/plain-f32": (3.67e-07, 0.0, 0.0),   # measured 3.6691e-07, 0, 0
    "sgd/plain-wd-bf16-cbf16": (4.19e-07, 0.0, 0.0),   # measured 4.1847e-07, 0, 0
    "sgd/plain-wdafter-f32": (4.89e-07, 0.0, 0.0),   # measured 4.8884e-07, 0, 0
    "sgd/nest-wd-f32": (3.41e-07, 6.67e-07, 0.0),   # measured 3.4032e-07, 6.6658e-07, 0
    "sgd/nest-wdafter-bf16-cbf16": (3.77e-07, 2.88e-07, 0.0),   # measured 3.7625e-07, 2.8729e-07, 0
    "sgd/mom-wd-f16-cf16": (4.8e-07, 1.27e-07, 0.0),   # measured 4.7913e-07, 1.2611e-07, 0
    "sgd/mom-damp-wd-f32": (5.57e-07, 6.06e-07, 0.0),   # measured 5.5673e-07, 6.0549e-07, 0
    "sgd/mom-damp-wdafter-f16": (4.5e-07, 4.43e-09, 0.0),   # measured 4.4981e-07, 4.4268e-09, 0
    "sgd/mom-f32-cbf16": (3.49e-07, 6.64e-07, 0.0),   # measured 3.4836e-07, 6.6393e-07, 0
    "sgd/mom-damp-wdafter-bf16-cbf16-many": (3.31e-07, 2.77e-07, 0.0),   # measured 3.3067e-07, 2.7692e-07, 0
    "sgd/nest-wd-f32-cf16-many": (4.58e-07, 7.64e-07, 0.0),   # measured 4.5753e-07, 7.6389e-07, 0
    "sgd/plain-wd-f16-many": (5.78e-07, 0.0, 0.0),   # measured 5.7732e-07, 0, 0
    "adam/adamw-f32": (5.26e-07, 6.2e-08, 3.51e-09),   # measured 5.2566e-07, 6.1942e-08, 3.5042e-09
    "adam/adamw-bf16-cbf16": (4.02e-07, 4.31e-10, 1.8e-13),   # measured 4.0138e-07, 4.3097e-10, 1.7996e-13
    "adam/l2-f32": (5.07e-07, 6.52e-08, 3.46e-09),   # measured 5.0676e-07, 6.5159e-08, 3.4594e-09
    "adam/l2-bf16-cbf16": (7.94e-07, 1.54e-09, 9.28e-13),   # measured 7.9346e-07, 1.5333e-09, 9.2717e-13
    "adam/l2-f32-cf16-nobc": (3.61e-06, 3.8e-08, 1.13e-09),   # measured 3.6048e-06, 3.7906e-08, 1.1291e-09
    "adam/adamw-bf16-cbf16-many": (6.74e-07, 4.17e-10, 1.62e-13),   # measured 6.7330e-07, 4.1694e-10, 1.6148e-13
    "adam/l2-f32-many": (6.16e-07, 5.98e-08, 3.47e-09),   # measured 6.1580e-07, 5.9735e-08, 3.4601e-09
    "adam/adamw-f32-clipamp": (4.16e-07, 1.11e-10, 7.66e-15),   # measured 4.1564e-07, 1.1068e-10, 7.6528e-15
    "lamb/bench-wd-adamw-clip": (4.34e-07, 3.75e-09, 7.79e-13),   # measured 4.3372e-07, 3.7486e-09, 7.7845e-13
    "lamb/f32-wd0-adamw-noclip": (5.83e-07, 5.32e-08, 3.3e-09),   # measured 5.8262e-07, 5.3118e-08, 3.2979e-09
    "lamb/f32-wd0-nvlamb-l2-clip-gnorm": (3.5e-07, 1.34e-09, 8.91e-15),   # measured 3.4906e-07, 1.3359e-09, 8.9089e-15
    "lamb/f32-wd-l2-noavg-noclip": (4.57e-07, 7.49e-07, 2.95e-09),   # measured 4.5689e-07, 7.4853e-07, 2.9478e-09
    "lamb/bench-wd-l2-noavg-gnorm-many": (1.53e-06, 2.89e-08, 1.24e-12),   # measured 1.5251e-06, 2.8833e-08, 1.2350e-12
    "lamb/f32-wd-adamw-nvlamb-clip-many": (3.92e-07, 9.99e-10, 2.22e-13),   # measured 3.9150e-07, 9.9848e-10, 2.2167e-13
}
# LARC, fp32 gradients and parameters: (rescaled gradient, stepped parameter) per
# (clip, weight decay != 0)
LARC_BOUNDS = {
    (True, False): (1.1e-07, 1.75e-07),   # measured 1.0932e-07, 1.7436e-07
    (True, True): (1.19e-07, 2.13e-07),   # measured 1.1805e-07, 2.1298e-07
    (False, False): (1.3e-08, 2.3e-07),   # measured 1.2971e-08, 2.2956e-07
    (False, True): (1.53e-08, 1.81e-07),   # measured 1.5299e-08, 1.8068e-07
}
