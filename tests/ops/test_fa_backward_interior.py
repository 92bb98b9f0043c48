"""Flash-attention backward with the mask-free interior body (and any later
reordering of a tile's work or widening of the epilogue stores): dq, dk and
dv must stay bit-identical to the build before that change, at the smallest
shapes where each such piece can go wrong (see the comment at each case).

The golden file holds what the earlier build computed; record_golden() below
wrote it (run by hand on that build, see profiles/r06_attn_bwd_valu.md)."""
import hashlib
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_E = torch.empty(0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                      "golden", "fa_backward_interior.npz")

# name: (b, sq, sk, h, hk, d, window, q_lens, k_lens, dtype, causal values)
_BF, _FP = torch.bfloat16, torch.float16
_BOTH = (False, True)
_NOWIN = (-1, -1)
_CASES = {
    # interior, diagonal and skipped waves in the same tile; odd and even
    # buffer hops; the head boundary
    "i01_s384_gqa": (1, 384, 384, 2, 1, 128, _NOWIN, None, None, _BF, _BOTH),
    # the last q tile and the last key block are partial (general body); the
    # epilogue row bounds are no multiple of 8
    "i02_s300": (1, 300, 300, 1, 1, 128, _NOWIN, None, None, _BF, _BOTH),
    # rows with no visible key: lse = -inf keeps those tiles off the fast path
    "i03_sq288_sk160": (1, 288, 160, 1, 1, 128, _NOWIN, None, None, _BF,
                        (True,)),
    # positive shift
    "i04_sq160_sk288": (1, 160, 288, 1, 1, 128, _NOWIN, None, None, _BF,
                        _BOTH),
    # cuts inside a tile and inside a wave's key block
    "i05_s320_lens": (2, 320, 320, 1, 1, 128, _NOWIN, [300, 131], [257, 77],
                      _BF, _BOTH),
    "i06_s320_left_window64": (1, 320, 320, 1, 1, 128, (64, -1), None, None,
                               _BF, _BOTH),
    "i07_s320_right_window40": (1, 320, 320, 1, 1, 128, (-1, 40), None, None,
                                _BF, (False,)),
    # the NA=2 schedule
    "i08_s320_d64": (1, 320, 320, 1, 1, 64, _NOWIN, None, None, _BF, _BOTH),
    "i09_s160_fp16": (1, 160, 160, 2, 1, 128, _NOWIN, None, None, _FP, _BOTH),
    # one key, and one 8-row group, into the second dkv workgroup
    "i10_sq64_sk129": (1, 64, 129, 1, 1, 128, _NOWIN, None, None, _BF, _BOTH),
    "i10_sq64_sk136": (1, 64, 136, 1, 1, 128, _NOWIN, None, None, _BF, _BOTH),
}
_PARAMS = [(name, causal) for name in sorted(_CASES)
           for causal in _CASES[name][10]]
# Raw 16-bit patterns are stored for a case whose three outputs are at most
# this many elements together; a larger case is stored as the SHA-256 of the
# same patterns (scheme of test_fa_backward_prefetch.py).
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


def _run_case(name, causal):
    b, sq, sk, h, hk, d, win, ql, kl, dtype, _ = _CASES[name]
    q, k, v, dout = _inputs(b, sq, sk, h, hk, d)
    ext = _ext()
    scale = 1.0 / math.sqrt(d)
    qg, kg, vg, dog = [t.to("cuda", dtype) for t in (q, k, v, dout)]
    qle = torch.tensor(ql, dtype=torch.int32) if ql is not None else _E
    kle = torch.tensor(kl, dtype=torch.int32) if kl is not None else _E
    o, lse = ext.fa_forward(qg, kg, vg, scale, causal, win[0], win[1], qle,
                            kle, _E, 0.0, 0)
    grads = ext.fa_backward(dog, qg, kg, vg, o, lse, scale, causal, win[0],
                            win[1], qle, kle, _E, 0.0, 0)
    return [g.cpu().contiguous().view(torch.int16).numpy() for g in grads]


def _digest(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


def record_golden(path=GOLDEN):
    """Run by hand on the build whose results are to be kept:
    python -c "from tests.ops.test_fa_backward_interior import record_golden
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
def test_fa_backward_interior_bit_identical(golden, name, causal):
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
