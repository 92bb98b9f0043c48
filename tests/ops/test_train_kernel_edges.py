"""Edge-shape numerics of the fused training kernels against float64.

Every case runs twice from one table: on the CPU (the composite path, which
validates the references, the case table and the bound without a GPU) and,
marked ``gpu``, through the HIP kernels on the same inputs. References and
the bound live in ``_train_refs``; shapes are the smallest that reach each
grid-stride second trip, vector-width tail and kernel-selection threshold.
"""
import pytest
import torch

from torchacc_amd.ops.adamw import AdamW
from torchacc_amd.ops.cross_entropy import _chunk_ce_forward, cross_entropy
from torchacc_amd.ops.rmsnorm import (_ref_rms_forward, fused_add_rms_norm,
                                      rms_norm)
from torchacc_amd.ops.rope import apply_rotary_pos_emb
from torchacc_amd.ops.swiglu import swiglu

from . import _train_refs as R

DEVICES = [pytest.param("cpu", id="cpu"),
           pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
DTYPES = [pytest.param(torch.bfloat16, id="bf16"),
          pytest.param(torch.float16, id="fp16")]
EPS = 1e-6


def _ext():
    from torchacc_amd.ops._backend import require_extension
    return require_extension()


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))
                  % (2 ** 31))
    return g


def _randn(*shape, g):
    """N(0,1) pushed 1/16 away from zero. fp16 results below 2^-14 are
    subnormal and carry up to 2^-25 of rounding error whatever their size,
    which the bound has no term for; with every input at least 1/16 in
    magnitude each ``scale`` stays above 2^-9 (2^-16 * 2^-9 = 2^-25) and a
    norm's y = x_hat * w stays a normal number or an exact zero."""
    t = torch.randn(*shape, generator=g)
    return t + torch.sign(t) / 16


def _leaf(t, device):
    """A fresh leaf on ``device`` (``.to`` alone aliases a CPU tensor)."""
    return t.detach().clone().to(device).requires_grad_(True)


def _bits(t):
    """Raw bits, so that -0.0 != 0.0 and NaNs compare."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


# --------------------------------------------------------------------------
# RMSNorm and add+RMSNorm
# --------------------------------------------------------------------------

NORM_SHAPES = [
    (1, 8),         # one active lane
    (3, 264),       # partial wave
    (513, 2056),    # backward grid cap; generic path past a fast width;
                    # second loop trip for thread 0
    (2049, 2048),   # forward grid cap; fast ITERS=1
    (513, 4096),    # fast ITERS=2; block 0 owns two rows of dw
    (5, 8192),      # fast ITERS=4
    (2049, 264),    # generic path, many rows per block
]


def _norm_inputs(rows, H, dtype, resid, tag):
    """x (and residual), weight, dy, dresid in ``dtype`` on the CPU.
    With >= 3 rows: row 0 is all zero (inv_rms = rsqrt(eps)), row 1 sits at
    5.9e4..6e4 (near the fp16 maximum; its dy is scaled by 2^10 so that its
    dx, of order dy / 6e4, stays a normal fp16 number). The weight has mixed
    sign and zeros."""
    g = _gen(rows, H, tag)
    x = _randn(rows, H, g=g)
    # the residual has x's sign: the sum must not cancel to a tiny value
    res = torch.sign(x) * _randn(rows, H, g=g).abs() if resid else None
    w = _randn(H, g=g)
    w[::5] = 0.0
    dy = _randn(rows, H, g=g)
    dres = _randn(rows, H, g=g)
    if rows >= 3:
        x[0] = 0.0
        sign = torch.where(torch.rand(H, generator=g) < 0.5, -1.0, 1.0)
        x[1] = sign * (6.0e4 - 1.0e3 * torch.rand(H, generator=g))
        dy[1] *= 1024.0
        if resid:
            res[0] = 0.0
            # same sign as x would pass the fp16 maximum
            res[1] = -sign * res[1].abs()
    cast = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    return cast(x), cast(res), cast(w), cast(dy), cast(dres)


def _norm_forward_raw(x, res, w, add):
    """(y, resid_out or None, inv_rms) from the entry point itself."""
    if x.is_cuda:
        ext = _ext()
        if add:
            empty = torch.empty(0, device=x.device, dtype=x.dtype)
            y, r, inv = ext.add_rmsnorm_forward(
                x, res if res is not None else empty, w, EPS)
            return y, r, inv
        y, inv = ext.rmsnorm_forward(x, w, EPS)
        return y, None, inv
    r = x + res if res is not None else x
    y, inv = _ref_rms_forward(r, w, EPS)
    return y, (r if add else None), inv.squeeze(-1)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["rms", "add", "add_noresid"])
@pytest.mark.parametrize("shape", NORM_SHAPES,
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_norm(shape, variant, dtype, device):
    rows, H = shape
    add = variant != "rms"
    x, res, w, dy, dres = _norm_inputs(rows, H, dtype, variant == "add", 1)
    r_exact = x + res if res is not None else x   # rounded in the dtype
    ref = R.rmsnorm_ref(r_exact, w, EPS, dy, dres if add else None)
    name = f"norm.{variant}"

    xd = _leaf(x, device)
    wd = _leaf(w, device)
    rd = _leaf(res, device) if res is not None else None
    if add:
        y, r = fused_add_rms_norm(xd, rd, wd, EPS)
        assert torch.equal(_bits(r), _bits(r_exact)), \
            "resid_out must be x + residual rounded in the tensor dtype"
        torch.autograd.backward([y, r], [dy.to(device), dres.to(device)])
    else:
        y = rms_norm(xd, wd, EPS)
        y.backward(dy.to(device))
    assert y.dtype == dtype and xd.grad.dtype == dtype
    assert wd.grad.dtype == dtype
    R.check(f"{name}.y", y, ref["y"], ref["y"].abs())
    R.check(f"{name}.dx", xd.grad, ref["dx"], ref["dx_scale"])
    R.check(f"{name}.dw", wd.grad, ref["dw"], ref["dw_scale"])
    if rd is not None:
        assert torch.equal(_bits(rd.grad), _bits(xd.grad))

    yr, rr, inv = _norm_forward_raw(x.to(device), None if res is None else
                                    res.to(device), w.to(device), add)
    assert inv.dtype == torch.float32 and inv.shape == (rows,)
    R.check(f"{name}.inv_rms", inv, ref["inv_rms"], R.unit(ref["inv_rms"]))
    assert torch.equal(_bits(yr), _bits(y))
    if add:
        assert torch.equal(_bits(rr), _bits(r_exact))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 264), (513, 2056), (513, 4096)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_add_norm_backward_without_dresid(shape, dtype, device):
    """The has_dresid=false branch: autograd always hands the function a
    (zero) residual gradient, so the entry point is called with an empty
    dresid; the CPU variant leaves the residual output out of the loss."""
    rows, H = shape
    x, res, w, dy, _ = _norm_inputs(rows, H, dtype, True, 2)
    r_exact = x + res
    ref = R.rmsnorm_ref(r_exact, w, EPS, dy, None)
    if device == "cuda":
        ext = _ext()
        _, r, inv = ext.add_rmsnorm_forward(x.cuda(), res.cuda(), w.cuda(),
                                            EPS)
        dx, dw = ext.add_rmsnorm_backward(
            dy.cuda(), torch.empty(0, device="cuda", dtype=dtype), r,
            w.cuda(), inv)
    else:
        xd = x.clone().requires_grad_(True)
        wd = w.clone().requires_grad_(True)
        y, _ = fused_add_rms_norm(xd, res, wd, EPS)
        y.backward(dy)
        dx, dw = xd.grad, wd.grad
    R.check("norm.add_nodresid.dx", dx, ref["dx"], ref["dx_scale"])
    R.check("norm.add_nodresid.dw", dw, ref["dw"], ref["dw_scale"])


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("shape", [(3, 261), (2049, 261)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_rmsnorm_fp32_forward(shape, device):
    rows, H = shape
    x, _, w, _, _ = _norm_inputs(rows, H, torch.float32, False, 3)
    ref = R.rmsnorm_ref(x, w, EPS)
    y, _, inv = _norm_forward_raw(x.to(device), None, w.to(device), False)
    assert y.dtype == torch.float32
    R.check("norm.fp32.y", y, ref["y"], ref["y"].abs())
    R.check("norm.fp32.inv_rms", inv, ref["inv_rms"], R.unit(ref["inv_rms"]))
    y2 = rms_norm(x.to(device), w.to(device), EPS)
    assert torch.equal(_bits(y2), _bits(y))


class _NormModule:
    """What utils.patch._patched_rmsnorm_forward is bound to."""

    def __init__(self, weight, eps):
        self.weight = weight
        self.variance_epsilon = eps


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", ["rms", "add", "patched"])
@pytest.mark.parametrize("shape", [(3, 264), (5, 2048)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_norm_fp32_weight(shape, entry, dtype, device):
    """16-bit activations with the weight kept in fp32 (autocast): same
    result as with the weight cast to the activation dtype, dw in fp32.
    The weight's values are rounded to the kernel dtype like every input."""
    from torchacc_amd.utils.patch import _patched_rmsnorm_forward
    rows, H = shape
    x, res, w, dy, dres = _norm_inputs(rows, H, dtype, entry == "add", 4)
    r_exact = x + res if res is not None else x
    ref = R.rmsnorm_ref(r_exact, w, EPS, dy, dres if entry == "add" else None)
    xd = _leaf(x, device)
    w32 = _leaf(w.float(), device)
    if entry == "add":
        y, r = fused_add_rms_norm(xd, res.to(device), w32, EPS)
        torch.autograd.backward([y, r], [dy.to(device), dres.to(device)])
    elif entry == "rms":
        y = rms_norm(xd, w32, EPS)
        y.backward(dy.to(device))
    else:
        y = _patched_rmsnorm_forward(_NormModule(w32, EPS), xd)
        y.backward(dy.to(device))
    assert y.dtype == dtype and w32.grad.dtype == torch.float32
    R.check(f"norm.w32.{entry}.y", y, ref["y"], ref["y"].abs())
    R.check(f"norm.w32.{entry}.dx", xd.grad, ref["dx"], ref["dx_scale"])
    R.check(f"norm.w32.{entry}.dw", w32.grad, ref["dw"], ref["dw_scale"])


# --------------------------------------------------------------------------
# SwiGLU
# --------------------------------------------------------------------------

SWIGLU_NUMEL = [
    8,                  # smallest legal size
    16,                 # 16-wide kernel
    24,                 # 8-wide kernel
    4194304 + 8,        # 8-wide kernel, second grid-stride trip
    8388608 + 48,       # 16-wide kernel, second trip
]


def _swiglu_inputs(n, dtype, tag):
    """Normal data with a block of extreme gate values at both ends, paired
    with small up / dy so that the float64 reference stays finite."""
    g = _gen(n, tag)
    gate = torch.randn(n, generator=g)
    up = _randn(n, g=g)
    dy = _randn(n, g=g)
    big = torch.finfo(dtype).max
    special = torch.tensor([big, -big, 100.0, -100.0, 88.0, -88.0, 0.0, -0.0,
                            20.0, -20.0])
    k = min(n, special.numel())
    # +-2^-4: max * 2^-4 is finite in both dtypes, dy * u = 2^-8 is normal
    gate[:k] = special[:k]
    up[:k] = torch.sign(up[:k]) / 16
    dy[:k] = torch.sign(dy[:k]) / 16
    if n >= 2 * k:
        gate[n - k:] = special[:k].flip(0)
        up[n - k:] = torch.sign(up[n - k:]) / 16
        dy[n - k:] = torch.sign(dy[n - k:]) / 16
    return gate.to(dtype), up.to(dtype), dy.to(dtype)


def _check_swiglu(name, gate, up, dy, run):
    ref = R.swiglu_ref(gate, up, dy)
    y, dg, du = run()
    R.check(f"{name}.y", y, ref["y"], ref["y_scale"])
    R.check(f"{name}.dg", dg, ref["dg"], ref["dg_scale"])
    R.check(f"{name}.du", du, ref["du"], ref["du_scale"])


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SWIGLU_NUMEL)
def test_swiglu(n, dtype, device):
    gate, up, dy = _swiglu_inputs(n, dtype, 1)

    def run():
        gd = _leaf(gate, device)
        ud = _leaf(up, device)
        y = swiglu(gd, ud)
        y.backward(dy.to(device))
        assert y.dtype == dtype
        return y, gd.grad, ud.grad

    _check_swiglu("swiglu", gate, up, dy, run)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 8), (6, 20), (5, 2, 16)],
                         ids=lambda s: "x".join(map(str, s)))
def test_swiglu_chunked_halves(shape, dtype, device):
    """gate / up as the two non-contiguous halves of one projection."""
    n = 1
    for s in shape:
        n *= s
    gate, up, dy = _swiglu_inputs(n, dtype, 2)
    gate, up, dy = gate.view(shape), up.view(shape), dy.view(shape)

    def run():
        fused = _leaf(torch.cat([gate, up], dim=-1), device)
        gd, ud = fused.chunk(2, dim=-1)
        assert not gd.is_contiguous()
        y = swiglu(gd, ud)
        y.backward(dy.to(device))
        dg, du = fused.grad.chunk(2, dim=-1)
        return y, dg, du

    _check_swiglu("swiglu.chunk", gate, up, dy, run)


# --------------------------------------------------------------------------
# RoPE
# --------------------------------------------------------------------------

ROPE_SHAPES = [
    (1, 1, 1, 1, 16),       # smallest legal shape
    (3, 5, 8, 2, 64),       # hq != hk
    (2, 300, 4, 4, 96),     # d/2 = 48
    (1, 7, 2, 1, 256),      # d = 256
    (2, 2100, 16, 2, 128),  # q passes 2048*256 work items, k does not
]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ROPE_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_rope(shape, dtype, device):
    b, s, hq, hk, d = shape
    g = _gen(*shape)
    q = _randn(b, s, hq, d, g=g).to(dtype)
    k = _randn(b, s, hk, d, g=g).to(dtype)
    dq = _randn(b, s, hq, d, g=g).to(dtype)
    dk = _randn(b, s, hk, d, g=g).to(dtype)
    # random tables, longer than s: a wrong row index cannot pass
    cos = torch.rand(s + 3, d // 2, generator=g) * 2 - 1
    sin = torch.rand(s + 3, d // 2, generator=g) * 2 - 1
    rq = R.rope_ref(q, cos, sin, dq)
    rk = R.rope_ref(k, cos, sin, dk)

    qd = _leaf(q, device)
    kd = _leaf(k, device)
    qo, ko = apply_rotary_pos_emb(qd, kd, cos.to(device), sin.to(device))
    torch.autograd.backward([qo, ko], [dq.to(device), dk.to(device)])
    assert qo.dtype == dtype and ko.dtype == dtype
    R.check("rope.q", qo, rq["out"], rq["out_scale"])
    R.check("rope.k", ko, rk["out"], rk["out_scale"])
    R.check("rope.dq", qd.grad, rq["dx"], rq["dx_scale"])
    R.check("rope.dk", kd.grad, rk["dx"], rk["dx_scale"])


# --------------------------------------------------------------------------
# cross-entropy
# --------------------------------------------------------------------------

CE_SHAPES = [(1, 5), (7, 8), (2049, 1003), (7, 2048), (7, 2056), (33, 5003),
             (7, 32000)]
IGNORE = -100
UPSTREAM = 3.5


def _ce_targets(rows, V, g):
    t = torch.randint(0, V, (rows,), generator=g)
    tail = V - (V % 8 or 8)          # first column of the last 8-chunk
    if rows >= 3:
        t[0], t[1], t[2] = 0, V - 1, tail
    else:
        t[0] = V - 1
    return t


def _ce_logits(rows, V, dtype, target, g):
    """Row i takes pattern i % 4: N(0,1); 30*N(0,1); a constant row; one
    column at 1e4 (bf16) / 6e4 (fp16) over N(0,1), on the target for every
    other such row."""
    x = torch.randn(rows, V, generator=g)
    big = 1.0e4 if dtype == torch.bfloat16 else 6.0e4
    for i in range(rows):
        kind = i % 4
        if kind == 1:
            x[i] *= 30.0
        elif kind == 2:
            x[i] = 1.5 - 0.25 * (i % 7)
        elif kind == 3:
            col = int(target[i]) if (i // 4) % 2 == 0 else (i * 7 + 3) % V
            x[i, col] = big
    return x.to(dtype)


def _ignore_patterns(rows, g):
    none = torch.zeros(rows, dtype=torch.bool)
    ends = none.clone()
    ends[0] = ends[-1] = True
    half = torch.rand(rows, generator=g) < 0.5
    return {"none": none, "ends": ends, "half": half,
            "all": torch.ones(rows, dtype=torch.bool)}


def _ce_forward_raw(logits, target):
    """(loss_sum, nvalid, lse) from the entry point itself."""
    ext = _ext() if logits.is_cuda else None
    return _chunk_ce_forward(ext, logits, target, IGNORE)


def _run_ce(name, logits, target, device, masked=None):
    ref = R.ce_ref(logits, target, IGNORE, UPSTREAM)
    ld = _leaf(logits, device)
    td = target.to(device)
    loss = cross_entropy(ld, td, IGNORE)
    (loss * UPSTREAM).backward()
    assert loss.dtype == torch.float32 and ld.grad.dtype == logits.dtype
    R.check(f"{name}.loss", loss, ref["loss"], R.unit(ref["loss"]))
    scale = ref["dlogits_scale"]
    if logits.dtype == torch.float16:
        # with more than 1792 valid rows the upstream scale 3.5 / nvalid is
        # below 2^-9 and every dlogits value is an fp16 subnormal (spacing
        # 2^-24): correct rounding alone errs by up to 2^-25 = 2^-16 * 2^-9
        scale = max(scale, 2.0 ** -9)
    R.check(f"{name}.dlogits", ld.grad, ref["dlogits"], scale)
    loss_sum, nvalid, lse = _ce_forward_raw(logits.to(device), td)
    assert int(nvalid) == ref["nvalid"]
    R.check(f"{name}.lse", lse, ref["lse"], R.unit(ref["lse"]))
    R.check(f"{name}.loss_sum", loss_sum.float(), ref["loss_sum"],
            R.unit(ref["loss_sum"]))
    if ref["nvalid"] == 0:
        assert float(loss.detach()) == 0.0
        assert not bool(ld.grad.float().cpu().any())
    if masked is not None:
        assert not bool(ld.grad.float().cpu()[masked].any()), \
            "dlogits must be exactly 0 on -inf columns"


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", CE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cross_entropy(shape, dtype, device):
    rows, V = shape
    g = _gen(rows, V, 1)
    target = _ce_targets(rows, V, g)
    logits = _ce_logits(rows, V, dtype, target, g)
    for kind, ign in _ignore_patterns(rows, g).items():
        _run_ce(f"ce.{kind}", logits, target.masked_fill(ign, IGNORE), device)


def _masked_sets(V):
    """-inf column sets; each leaves at least two finite columns."""
    sets = {"col0": [0]}
    if V > 10:
        sets["cols0-7"] = list(range(8))
    if V > 520:
        sets["wave1"] = list(range(512, min(1024, V)))  # wave 1's first slice
    if V % 8 and V > V % 8 + 2:
        sets["tail"] = list(range(V - V % 8, V))
    sets["all_but_two"] = None
    return sets


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", CE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cross_entropy_masked_logits(shape, dtype, device):
    """Vocabulary masking: -inf columns, the target on a finite one. The loss
    is finite and equals the reference; dlogits is exactly 0 where masked."""
    rows, V = shape
    g = _gen(rows, V, 2)
    base = torch.randn(rows, V, generator=g)
    for kind, cols in _masked_sets(V).items():
        mask = torch.zeros(rows, V, dtype=torch.bool)
        if cols is None:
            keep = torch.stack([torch.randperm(V, generator=g)[:2]
                                for _ in range(rows)])
            mask[:] = True
            mask.scatter_(1, keep, False)
        else:
            mask[:, cols] = True
        # a random finite column per row
        finite = (~mask).float()
        target = torch.multinomial(finite, 1, generator=g).squeeze(1)
        logits = base.masked_fill(mask, float("-inf")).to(dtype)
        _run_ce(f"ce.masked.{kind}", logits, target, device, masked=mask)


# --------------------------------------------------------------------------
# AdamW
# --------------------------------------------------------------------------

ADAM_SIZES = [1, 3, 4, 5, 1023, 1027,
              2097159]      # second grid-stride trip plus a 3-element tail
ADAM_MODES = [
    pytest.param((torch.bfloat16, True), id="bf16-master"),
    pytest.param((torch.float16, True), id="fp16-master"),
    pytest.param((torch.bfloat16, False), id="bf16-nomaster"),
    pytest.param((torch.float16, False), id="fp16-nomaster"),
    pytest.param((torch.float32, False), id="fp32"),
]
ADAM_HYPER = [
    pytest.param(dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8,
                      weight_decay=0.1), id="default-wd0.1"),
    pytest.param(dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-5,
                      weight_decay=0.0), id="betas-wd0"),
]


def _adam_grad(n, dtype, g):
    grad = torch.randn(n, generator=g)
    grad[::3] = 0.0           # v stays 0 there: the denominator is eps
    return grad.to(dtype)


def _adam_state(opt, p):
    st = opt.state[p]
    return [p, st["exp_avg"], st["exp_avg_sq"]] + (
        [st["master"]] if "master" in st else [])


def _check_adam(name, opt, p, ref_p, ref_m, ref_v, master):
    st = opt.state[p]
    R.check(f"{name}.exp_avg", st["exp_avg"], ref_m, R.unit(ref_m))
    R.check(f"{name}.exp_avg_sq", st["exp_avg_sq"], ref_v, R.unit(ref_v))
    if master:
        R.check(f"{name}.master", st["master"], ref_p, R.unit(ref_p))
    else:
        assert "master" not in st
    # the parameter: one ulp of its dtype around the (master) value
    R.check(f"{name}.param", p, ref_p, R.unit(ref_p))


def _check_skipped_step(opt, params, device):
    """found_inf = 1: nothing may change, bit for bit."""
    before = [[_bits(t).clone() for t in _adam_state(opt, p)] for p in params]
    opt.step(found_inf=torch.ones((), dtype=torch.float32, device=device))
    for p, old in zip(params, before):
        for t, o in zip(_adam_state(opt, p), old):
            assert torch.equal(_bits(t), o)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("hyper", ADAM_HYPER)
@pytest.mark.parametrize("mode", ADAM_MODES)
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adamw(n, mode, hyper, device):
    dtype, master = mode
    g = _gen(n, 1)
    p0 = torch.randn(n, generator=g).to(dtype)
    p = _leaf(p0, device)
    opt = AdamW([p], use_master_weights=master, **hyper)
    h = (hyper["lr"], *hyper["betas"], hyper["eps"], hyper["weight_decay"])
    rp = R.wide(p0)
    if master or dtype == torch.float32:
        # three steps from zero state; the reference never rounds
        rm = torch.zeros_like(rp)
        rv = torch.zeros_like(rp)
        for step in (1, 2, 3):
            grad = _adam_grad(n, dtype, g)
            p.grad = grad.to(device)
            opt.step()
            rp, rm, rv = R.adamw_ref_step(rp, R.wide(grad), rm, rv, step, *h)
    else:
        # one step (the third) from identical, non-trivial state: without
        # master weights the parameter is re-rounded after every step
        m0 = 0.1 * torch.randn(n, generator=g)
        v0 = 0.01 * torch.rand(n, generator=g)
        opt.state[p] = {"step": 2.0, "exp_avg": m0.clone().to(device),
                        "exp_avg_sq": v0.clone().to(device)}
        grad = _adam_grad(n, dtype, g)
        p.grad = grad.to(device)
        opt.step()
        rp, rm, rv = R.adamw_ref_step(rp, R.wide(grad), R.wide(m0),
                                      R.wide(v0), 3, *h)
    assert opt.state[p]["step"] == 3.0
    _check_adam("adamw", opt, p, rp, rm, rv, master)
    _check_skipped_step(opt, [p], device)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("mode", ADAM_MODES)
def test_adamw_per_parameter_steps(mode, device):
    """One step() over three parameters whose step counts differ: the second
    has no grad on the first step."""
    dtype, master = mode
    hyper = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.1)
    h = (hyper["lr"], *hyper["betas"], hyper["eps"], hyper["weight_decay"])
    g = _gen(dtype.itemsize, int(master), 7)
    sizes = [5, 1027, 4]
    p0 = [torch.randn(n, generator=g).to(dtype) for n in sizes]
    ps = [_leaf(t, device) for t in p0]
    opt = AdamW(ps, use_master_weights=master, **hyper)
    ref = [(R.wide(t), torch.zeros(n, dtype=torch.float64),
            torch.zeros(n, dtype=torch.float64)) for t, n in zip(p0, sizes)]
    steps = [0, 0, 0]
    for it in range(2):
        for i, p in enumerate(ps):
            if it == 0 and i == 1:
                p.grad = None
                continue
            grad = _adam_grad(sizes[i], dtype, g)
            p.grad = grad.to(device)
            steps[i] += 1
            ref[i] = R.adamw_ref_step(ref[i][0], R.wide(grad), ref[i][1],
                                      ref[i][2], steps[i], *h)
            if not master and dtype != torch.float32:
                ref[i] = (R.wide(ref[i][0].to(dtype)),) + ref[i][1:]
        opt.step()
    assert [opt.state[p]["step"] for p in ps] == [2.0, 1.0, 2.0]
    for i, p in enumerate(ps):
        _check_adam("adamw.multi", opt, p, *ref[i], master)
    _check_skipped_step(opt, ps, device)


# --------------------------------------------------------------------------
# host checks: each raises before any kernel is launched
# --------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_checks(dtype):
    ext = _ext()
    dev = "cuda"

    def t(*shape, dt=dtype):
        return torch.ones(*shape, device=dev, dtype=dt)

    empty = torch.empty(0, device=dev, dtype=dtype)
    inv = t(3, dt=torch.float32)
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    calls = {
        # hidden size not a multiple of 8
        "rms H%8": lambda: rms_norm(t(3, 12), t(12), EPS),
        "add H%8": lambda: fused_add_rms_norm(t(3, 12), t(3, 12), t(12), EPS),
        "rms bwd H%8": lambda: ext.rmsnorm_backward(
            t(3, 12), t(3, 12), t(12), inv),
        "add bwd H%8": lambda: ext.add_rmsnorm_backward(
            t(3, 12), empty, t(3, 12), t(12), inv),
        # weight numel != H
        "rms w": lambda: rms_norm(t(3, 16), t(8), EPS),
        "add w": lambda: fused_add_rms_norm(t(3, 16), None, t(24), EPS),
        "rms bwd w": lambda: ext.rmsnorm_backward(
            t(3, 16), t(3, 16), t(8), inv),
        "add bwd w": lambda: ext.add_rmsnorm_backward(
            t(3, 16), empty, t(3, 16), t(32), inv),
        # backward dtype / shape
        "rms bwd dy dtype": lambda: ext.rmsnorm_backward(
            t(3, 16, dt=torch.float32), t(3, 16), t(16), inv),
        "add bwd dy dtype": lambda: ext.add_rmsnorm_backward(
            t(3, 16, dt=torch.float32), empty, t(3, 16), t(16), inv),
        "add bwd fp32": lambda: ext.add_rmsnorm_backward(
            t(3, 16, dt=torch.float32), empty, t(3, 16, dt=torch.float32),
            t(16, dt=torch.float32), inv),
        "add bwd dresid": lambda: ext.add_rmsnorm_backward(
            t(3, 16), t(3, 16, dt=other), t(3, 16), t(16), inv),
        "add bwd dy shape": lambda: ext.add_rmsnorm_backward(
            t(2, 16), empty, t(3, 16), t(16), inv),
        # swiglu
        "swiglu fwd %8": lambda: ext.swiglu_forward(t(12), t(12)),
        "swiglu fwd u shape": lambda: ext.swiglu_forward(t(16), t(8)),
        "swiglu fwd u dtype": lambda: ext.swiglu_forward(t(16),
                                                         t(16, dt=other)),
        "swiglu bwd %8": lambda: ext.swiglu_backward(t(12), t(12), t(12)),
        "swiglu bwd u shape": lambda: ext.swiglu_backward(
            t(16), t(16), t(8)),
        "swiglu bwd u dtype": lambda: ext.swiglu_backward(
            t(16), t(16), t(16, dt=other)),
        "swiglu bwd dy shape": lambda: ext.swiglu_backward(
            t(32), t(16), t(16)),
        "swiglu bwd dy dtype": lambda: ext.swiglu_backward(
            t(16, dt=torch.float32), t(16), t(16)),
        # rope head_dim
        "rope d%16": lambda: apply_rotary_pos_emb(
            t(1, 2, 1, 24), t(1, 2, 1, 24), t(2, 12, dt=torch.float32),
            t(2, 12, dt=torch.float32)),
        # int32 targets
        "ce int32": lambda: ext.cross_entropy_forward(
            t(3, 16), torch.zeros(3, device=dev, dtype=torch.int32), IGNORE),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"{name}: no error raised")
    torch.cuda.synchronize()
