"""Flash-attention backward with double-buffered staging and the dual-use
LDS images: edge shapes against the fp32 reference, the plain path against
the structurally older alibi/dropout clone, and run-to-run determinism at a
shape that fills every CU with several workgroups."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

_E = torch.empty(0)


def _ext():
    from torchacc_amd.ops._backend import require_extension
    return require_extension()


def _inputs(b, sq, sk, h, hk, d, seed=0):
    torch.manual_seed(seed)
    q = torch.randn(b, sq, h, d)
    k = torch.randn(b, sk, hk, d)
    v = torch.randn(b, sk, hk, d)
    dout = torch.randn(b, sq, h, d)
    return q, k, v, dout


def _visible_rows(b, sq, sk, causal, window, k_lens):
    """[b, 1, sq] bool: the q row has at least one unmasked key."""
    iq = torch.arange(sq).view(1, sq, 1)
    ik = torch.arange(sk).view(1, 1, sk)
    shift = sk - sq
    ok = torch.ones(b, sq, sk, dtype=torch.bool)
    if causal:
        ok &= ik <= iq + shift
    wl, wr = window
    if wl >= 0:
        ok &= ik >= iq + shift - wl
    if wr >= 0 and not causal:
        ok &= ik <= iq + shift + wr
    if k_lens is not None:
        ok &= ik < k_lens.view(b, 1, 1)
    return ok.any(-1).view(b, 1, sq)


# (b, sq, sk, h, hk, d, window, q_lens, k_lens, dtype)
_REF_CASES = {
    "s33_two_q_tiles": (1, 33, 33, 2, 2, 128, (-1, -1), None, None,
                        torch.bfloat16),
    "s96_odd_tile_count": (2, 96, 96, 2, 2, 128, (-1, -1), None, None,
                           torch.bfloat16),
    "s160_gqa4": (1, 160, 160, 8, 2, 128, (-1, -1), None, None,
                  torch.bfloat16),
    "sq160_sk288": (1, 160, 288, 2, 2, 128, (-1, -1), None, None,
                    torch.bfloat16),
    "sq288_sk160": (1, 288, 160, 2, 2, 128, (-1, -1), None, None,
                    torch.bfloat16),
    "s192_d64": (2, 192, 192, 4, 4, 64, (-1, -1), None, None,
                 torch.bfloat16),
    "s320_lens": (2, 320, 320, 2, 2, 128, (-1, -1), [300, 131], [257, 77],
                  torch.bfloat16),
    "s320_window64": (1, 320, 320, 2, 2, 128, (64, -1), None, None,
                      torch.bfloat16),
    "s160_fp16": (1, 160, 160, 4, 2, 128, (-1, -1), None, None,
                  torch.float16),
}


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", sorted(_REF_CASES))
def test_fa_backward_pipeline_vs_reference(case, causal):
    """Same measure and bound as test_fa_backward: max error over max
    magnitude < 4e-2 against the fp32 composite."""
    from torchacc_amd.ops.flash_attn import (_ref_attention,
                                             _ref_fa_backward)
    ext = _ext()
    b, sq, sk, h, hk, d, win, ql, kl, dtype = _REF_CASES[case]
    q, k, v, dout = _inputs(b, sq, sk, h, hk, d)
    scale = 1.0 / math.sqrt(d)
    qlt = torch.tensor(ql, dtype=torch.int32) if ql is not None else None
    klt = torch.tensor(kl, dtype=torch.int32) if kl is not None else None
    if qlt is not None or klt is not None:
        ref_o, ref_lse = _ref_attention(q, k, v, scale, causal, win, qlt,
                                        klt)
    else:
        ref_o, ref_lse = _ref_attention(q, k, v, scale, causal, win)
    # A q row that sees no key (causal with sq > sk) has no softmax: the
    # kernels give it zero gradient, while the composite's exp(score - lse)
    # is not defined there. lse = +inf makes its p exactly 0 in the composite
    # as well, so the row drops out of dq, dk and dv on both sides.
    ref_lse = torch.where(_visible_rows(b, sq, sk, causal, win, klt),
                          ref_lse, torch.full_like(ref_lse, float("inf")))
    rdq, rdk, rdv = _ref_fa_backward(dout, q, k, v, ref_o, ref_lse, scale,
                                     causal, win, qlt, klt)
    qg, kg, vg, dog = [t.to("cuda", dtype) for t in (q, k, v, dout)]
    qle = qlt if qlt is not None else _E
    kle = klt if klt is not None else _E
    o, lse = ext.fa_forward(qg, kg, vg, scale, causal, win[0], win[1], qle,
                            kle, _E, 0.0, 0)
    dq, dk, dv = ext.fa_backward(dog, qg, kg, vg, o, lse, scale, causal,
                                 win[0], win[1], qle, kle, _E, 0.0, 0)
    for name, got, want in (("dq", dq, rdq), ("dk", dk, rdk),
                            ("dv", dv, rdv)):
        err = (got.float().cpu() - want.float()).abs().max()
        base = want.float().abs().max().clamp_min(1.0)
        print(f"{case} causal={causal} {name}: err/base = "
              f"{float(err / base):.4g}")
        assert err / base < 4e-2, f"{name} err {err} (max {base})"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", [
    (1, 4096, 4, 4, 128),
    (2, 1024, 8, 2, 128),
])
def test_fa_backward_pipeline_vs_clone(shape, causal):
    """alibi_slopes = 0 routes fa_backward to the alibi/dropout clone, which
    keeps the single-buffered structure and the same rounding points, so the
    two paths stay within the few bf16 ulps they were apart before the plain
    path was pipelined (_CLONE_BOUND)."""
    ext = _ext()
    b, s, h, hk, d = shape
    q, k, v, dout = _inputs(b, s, s, h, hk, d, seed=1)
    scale = 1.0 / math.sqrt(d)
    qg, kg, vg, dog = [t.to("cuda", torch.bfloat16)
                       for t in (q, k, v, dout)]
    o, lse = ext.fa_forward(qg, kg, vg, scale, causal, -1, -1, _E, _E, _E,
                            0.0, 0)
    plain = ext.fa_backward(dog, qg, kg, vg, o, lse, scale, causal, -1, -1,
                            _E, _E, _E, 0.0, 0)
    slopes = torch.zeros(h, device="cuda", dtype=torch.float32)
    clone = ext.fa_backward(dog, qg, kg, vg, o, lse, scale, causal, -1, -1,
                            _E, _E, slopes, 0.0, 0)
    diffs = {name: float((a.float() - c.float()).abs().max())
             for name, a, c in zip(("dq", "dk", "dv"), plain, clone)}
    print(f"{shape} causal={causal} max |plain - clone|: {diffs}")
    for name, diff in diffs.items():
        assert diff <= _CLONE_BOUND, f"{name} differs from clone by {diff}"


# Largest |plain - clone| over dq/dk/dv and the four cases above, measured
# on the parent commit (single-buffered plain path): 0.00390625, one bf16 ulp
# of a gradient in [0.5, 1) (dk at (2, 1024, 8, 2, 128) causal; per case the
# maxima were 0.00049 / 0.00195 / 0.00195 / 0.00391). The clone adds the zero
# alibi bias to the score before the exp, so the two paths are a few ulps
# apart rather than equal. The bound is that value with a 2x margin.
_CLONE_BOUND = 2 * 0.00390625


@pytest.mark.parametrize("causal", [False, True])
def test_fa_backward_pipeline_deterministic(causal):
    """Three calls on the same inputs must agree bit for bit: a staging race
    between the two LDS buffers shows as run-to-run noise at a shape that
    keeps several workgroups on every CU."""
    ext = _ext()
    b, s, h, hk, d = 2, 4096, 8, 8, 128
    torch.manual_seed(2)
    dev = "cuda"
    q = torch.randn(b, s, h, d, device=dev, dtype=torch.bfloat16)
    k = torch.randn(b, s, hk, d, device=dev, dtype=torch.bfloat16)
    v = torch.randn(b, s, hk, d, device=dev, dtype=torch.bfloat16)
    dout = torch.randn(b, s, h, d, device=dev, dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(d)
    o, lse = ext.fa_forward(q, k, v, scale, causal, -1, -1, _E, _E, _E,
                            0.0, 0)
    runs = [ext.fa_backward(dout, q, k, v, o, lse, scale, causal, -1, -1,
                            _E, _E, _E, 0.0, 0) for _ in range(3)]
    for i in (1, 2):
        for name, a, c in zip(("dq", "dk", "dv"), runs[0], runs[i]):
            assert torch.equal(a, c), f"{name} differs between call 0 and {i}"
    for name, a in zip(("dq", "dk", "dv"), runs[0]):
        assert torch.isfinite(a.float()).all(), f"{name} not finite"
