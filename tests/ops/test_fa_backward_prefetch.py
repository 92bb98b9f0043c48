"""Flash-attention backward with the direct-to-LDS prefetch in fa_bwd_dkv and
the pipelined transposed reads: dq, dk and dv must stay bit-identical to the
build before that change, at the smallest shapes where the new staging can go
wrong (clamped pad rows, buffer hops, head boundary, D=64, fp16, window, lens).

The golden file holds what the earlier build computed; record_golden() below
wrote it (run by hand on that build, see profiles/r05_attn_bwd_prefetch.md)."""
import hashlib
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_E = torch.empty(0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                      "golden", "fa_backward_prefetch.npz")

# name: (b, sq, sk, h, hk, d, window, q_lens, k_lens, dtype, causal values)
_BF, _FP = torch.bfloat16, torch.float16
_BOTH = (False, True)
_CASES = {
    "c1_s17_single_tile": (1, 17, 17, 1, 1, 128, (-1, -1), None, None, _BF,
                           _BOTH),
    "c2_s33_two_tiles": (1, 33, 33, 1, 1, 128, (-1, -1), None, None, _BF,
                         _BOTH),
    "c3_s96_b2_three_tiles": (2, 96, 96, 1, 1, 128, (-1, -1), None, None,
                              _BF, _BOTH),
    "c4_s72_gqa4_head_boundary": (1, 72, 72, 8, 2, 128, (-1, -1), None, None,
                                  _BF, _BOTH),
    "c5_sq100_sk230": (1, 100, 230, 1, 1, 128, (-1, -1), None, None, _BF,
                       _BOTH),
    "c5_sq230_sk100": (1, 230, 100, 1, 1, 128, (-1, -1), None, None, _BF,
                       _BOTH),
    "c6_s136_d64": (1, 136, 136, 1, 1, 64, (-1, -1), None, None, _BF, _BOTH),
    "c7_s40_fp16": (1, 40, 40, 2, 1, 128, (-1, -1), None, None, _FP, _BOTH),
    "c8_s200_window64": (1, 200, 200, 1, 1, 128, (64, -1), None, None, _BF,
                         (False,)),
    "c9_s200_lens": (2, 200, 200, 1, 1, 128, (-1, -1), [200, 77], [131, 200],
                     _BF, (False,)),
}
_PARAMS = [(name, causal) for name in sorted(_CASES)
           for causal in _CASES[name][10]]
# Raw 16-bit patterns are stored for a case whose three outputs are at most
# this many elements together; a larger case is stored as the SHA-256 of the
# same patterns, which keeps the file far below the size limit for a committed
# file and still fails on any changed bit.
_RAW_LIMIT = 30000


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


def _backward(ext, q, k, v, dout, dtype, causal, win=(-1, -1), ql=None,
              kl=None):
    d = q.shape[-1]
    scale = 1.0 / math.sqrt(d)
    qg, kg, vg, dog = [t.to("cuda", dtype) for t in (q, k, v, dout)]
    qle = torch.tensor(ql, dtype=torch.int32) if ql is not None else _E
    kle = torch.tensor(kl, dtype=torch.int32) if kl is not None else _E
    o, lse = ext.fa_forward(qg, kg, vg, scale, causal, win[0], win[1], qle,
                            kle, _E, 0.0, 0)
    grads = ext.fa_backward(dog, qg, kg, vg, o, lse, scale, causal, win[0],
                            win[1], qle, kle, _E, 0.0, 0)
    return grads, o, lse


def _run_case(name, causal):
    b, sq, sk, h, hk, d, win, ql, kl, dtype, _ = _CASES[name]
    q, k, v, dout = _inputs(b, sq, sk, h, hk, d)
    grads, _, _ = _backward(_ext(), q, k, v, dout, dtype, causal, win, ql,
                            kl)
    return [g.cpu().contiguous().view(torch.int16).numpy() for g in grads]


def _digest(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


def record_golden(path=GOLDEN):
    """Run by hand on the build whose results are to be kept:
    python -c "from tests.ops.test_fa_backward_prefetch import record_golden
    as r; r()" """
    out = {}
    for name, causal in _PARAMS:
        arrs = _run_case(name, causal)
        raw = sum(a.size for a in arrs) <= _RAW_LIMIT
        for tname, arr in zip(("dq", "dk", "dv"), arrs):
            key = f"{name}/causal={int(causal)}/{tname}"
            out[key] = arr if raw else np.array(_digest(arr))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    return path


@pytest.fixture(scope="module")
def golden():
    assert os.path.exists(GOLDEN), f"golden file missing: {GOLDEN}"
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name,causal", _PARAMS)
def test_fa_backward_prefetch_bit_identical(golden, name, causal):
    arrs = _run_case(name, causal)
    for tname, arr in zip(("dq", "dk", "dv"), arrs):
        want = golden[f"{name}/causal={int(causal)}/{tname}"]
        if want.dtype == np.int16:
            same = torch.equal(torch.from_numpy(arr), torch.from_numpy(want))
            ndiff = int((arr != want).sum()) if arr.shape == want.shape else -1
            assert same, f"{tname}: {ndiff} of {arr.size} patterns differ"
        else:
            assert _digest(arr) == str(want), \
                f"{tname}: bit patterns differ from the recorded build"


@pytest.mark.parametrize("causal", [False, True])
def test_fa_backward_prefetch_clamped_rows(causal):
    """sq = 33: the second 32-row tile has one real row and 31 pad rows, which
    the prefetch fills from the clamped source row sq-1, so whatever that row
    holds sits in LDS 32 times. P and dS of the pad rows are masked to 0; a
    pad row that leaked would add its products to dk and dv again.

    The last row of Q and dO is made large, but not the largest finite bf16:
    with 3.39e38 in Q the row's own score Q.K overflows fp32 in the kernels
    and in the fp32 composite alike (CPU check: _ref_fa_backward returns NaN
    in dk and dv for it), so no build can give finite gradients there and
    there is nothing to compare with. The values used are the largest powers
    of two that keep the REAL row's arithmetic well defined:
      Q[32] = 8: its scores are 8 * sum_d k_d * scale, std about 8, so that
        exp(score - lse) is still resolved in fp32 (a score near 1e4 or more
        has an ulp that no longer resolves the softmax, and forward and
        backward kernels need not round the score the same way);
      dO[32] = 2^100: dP, delta, dS and the products dS^T Q, P^T dO are
        linear in it and stay below 2^100 * 128 * 8 * 8 < 2^120 < fp32 max.
    That row's contribution then dominates dk and dv by about 2^100, so one
    leaked pad row doubles them (err/base about 1). Measure and bound as in
    test_fa_backward_pipeline_vs_reference, over all rows but the last."""
    from torchacc_amd.ops.flash_attn import _ref_fa_backward
    b, sq, sk, h, hk, d = 1, 33, 33, 1, 1, 128
    q, k, v, dout = _inputs(b, sq, sk, h, hk, d)
    q[:, -1] = 8.0
    dout[:, -1] = 2.0 ** 100
    q, k, v, dout = [t.bfloat16().float() for t in (q, k, v, dout)]
    scale = 1.0 / math.sqrt(d)
    (dq, dk, dv), o, lse = _backward(_ext(), q, k, v, dout, torch.bfloat16,
                                     causal)
    # the composite gets the kernels' own out and lse, as fa_backward does
    rdq, rdk, rdv = _ref_fa_backward(dout, q, k, v, o.float().cpu(),
                                     lse.float().cpu(), scale, causal,
                                     (-1, -1), None, None)
    for name, got, want in (("dq", dq, rdq), ("dk", dk, rdk),
                            ("dv", dv, rdv)):
        got = got.float().cpu()
        assert torch.isfinite(got).all(), f"{name} not finite"
        err = (got[:, :-1] - want.float()[:, :-1]).abs().max()
        base = want.float()[:, :-1].abs().max().clamp_min(1.0)
        print(f"clamped rows causal={causal} {name}: err/base = "
              f"{float(err / base):.4g}")
        assert err / base < 4e-2, f"{name} err {err} (max {base})"
