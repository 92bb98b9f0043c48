"""Heavy-first workgroup order of the causal attention kernels
(attn_wg_coord, csrc/attn_common.h): the order only decides which block
computes which (tile, batch-head), so it can go wrong at the edges of the
grid and nowhere else. Small awkward grids: one tile, batch-head counts that
are no multiple of 8 or of the chunk, a short last chunk, partial last tiles,
a causal shift in both directions.

Per case: forward (out, lse) and backward (dq, dk, dv) against the fp32
composite at the bounds of test_fa_forward / test_fa_backward, every row
compared (a tile skipped or visited twice shows there), two calls
bit-identical, and all five outputs bit-identical to the build before the
order changed. The golden file holds what that build computed;
record_golden() below wrote it (run by hand on that build, see
profiles/r13_attn_wg_order.md)."""
import functools
import hashlib
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_E = torch.empty(0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                      "golden", "fa_wg_order.npz")

_BF, _FP = torch.bfloat16, torch.float16
_NOWIN = (-1, -1)
# name: (b, sq, sk, h, hk, d, causal, window, k_lens, dtype)
_CASES = {
    # one tile, one batch-head
    "w01_b1_h1_s100": (1, 100, 100, 1, 1, 128, True, _NOWIN, None, _BF),
    # gridDim.y no multiple of 8; the last 128- and 256-row tiles are partial
    "w02_b1_h3_s300": (1, 300, 300, 3, 3, 128, True, _NOWIN, None, _BF),
    "w02_b1_h3_s300_fp16": (1, 300, 300, 3, 3, 128, True, _NOWIN, None, _FP),
    # 10 batch-heads: a short last chunk at a chunk of 8
    "w03_b2_h5_d64_s640": (2, 640, 640, 5, 5, 64, True, _NOWIN, None, _BF),
    # GQA: 24 forward/dq batch-heads, 6 dkv batch-heads
    "w04_b3_h8_hk2_s520": (3, 520, 520, 8, 2, 128, True, _NOWIN, None, _BF),
    # causal shift, both directions (the second has q rows that see no key)
    "w05_sq200_sk456": (2, 200, 456, 4, 4, 128, True, _NOWIN, None, _BF),
    "w05_sq456_sk200": (2, 456, 200, 4, 4, 128, True, _NOWIN, None, _BF),
    # the other instantiations at one awkward grid
    "w06_noncausal": (2, 300, 300, 3, 3, 128, False, _NOWIN, None, _BF),
    "w06_window64": (2, 300, 300, 3, 3, 128, True, (64, -1), None, _BF),
    "w06_klens": (2, 300, 300, 3, 3, 128, True, _NOWIN, [257, 77], _BF),
    # more batch-heads than any chunk of 8 or 16, and no multiple of it
    "w07_b19_h1_s260": (19, 260, 260, 1, 1, 128, True, _NOWIN, None, _BF),
}
_NAMES = sorted(_CASES)
_OUTS = ("out", "lse", "dq", "dk", "dv")
# Raw bit patterns are stored for a case whose five outputs are at most this
# many elements together; a larger case is stored as the SHA-256 of the same
# patterns (scheme of test_fa_backward_prefetch.py).
_RAW_LIMIT = 60000


def _ext():
    from torchacc_amd.ops._backend import require_extension
    return require_extension()


def _inputs(name):
    b, sq, sk, h, hk, d = _CASES[name][:6]
    torch.manual_seed(0)
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
    if window[0] >= 0:
        ok &= ik >= iq + shift - window[0]
    if k_lens is not None:
        ok &= ik < k_lens.view(b, 1, 1)
    return ok.any(-1).view(b, 1, sq)


def _gpu_run(name):
    """One forward and one backward call; the five outputs on the CPU."""
    b, sq, sk, h, hk, d, causal, win, kl, dtype = _CASES[name]
    ext = _ext()
    scale = 1.0 / math.sqrt(d)
    qg, kg, vg, dog = [t.to("cuda", dtype) for t in _inputs(name)]
    kle = torch.tensor(kl, dtype=torch.int32) if kl is not None else _E
    o, lse = ext.fa_forward(qg, kg, vg, scale, causal, win[0], win[1], _E,
                            kle, _E, 0.0, 0)
    dq, dk, dv = ext.fa_backward(dog, qg, kg, vg, o, lse, scale, causal,
                                 win[0], win[1], _E, kle, _E, 0.0, 0)
    return dict(zip(_OUTS, (t.cpu().contiguous()
                            for t in (o, lse, dq, dk, dv))))


@functools.lru_cache(maxsize=None)
def _runs(name):
    """Two independent GPU runs of a case, shared by its tests."""
    return _gpu_run(name), _gpu_run(name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """fp32 composite, computed once per case: (out, lse, dq, dk, dv, vis)."""
    from torchacc_amd.ops.flash_attn import _ref_attention, _ref_fa_backward
    b, sq, sk, h, hk, d, causal, win, kl, _ = _CASES[name]
    q, k, v, dout = _inputs(name)
    scale = 1.0 / math.sqrt(d)
    klt = torch.tensor(kl, dtype=torch.int32) if kl is not None else None
    ro, rlse = _ref_attention(q, k, v, scale, causal, win, None, klt)
    vis = _visible_rows(b, sq, sk, causal, win, klt)
    # a q row that sees no key: the kernels give it zero gradient; lse = +inf
    # makes its p exactly 0 in the composite as well
    # (test_fa_backward_pipeline.py)
    blse = torch.where(vis, rlse, torch.full_like(rlse, float("inf")))
    rdq, rdk, rdv = _ref_fa_backward(dout, q, k, v, ro, blse, scale, causal,
                                     win, None, klt)
    return ro, rlse, rdq, rdk, rdv, vis


def _patterns(name, t):
    """The raw bits of an output as a numpy integer array."""
    it = torch.int32 if name == "lse" else torch.int16
    return t.view(it).numpy()


def _digest(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


def record_golden(path=GOLDEN):
    """Run by hand on the build whose results are to be kept:
    python -c "from tests.ops.test_fa_wg_order import record_golden as r;
    r()" """
    out = {}
    for name in _NAMES:
        res = _gpu_run(name)
        raw = sum(t.numel() for t in res.values()) <= _RAW_LIMIT
        for tname in _OUTS:
            arr = _patterns(tname, res[tname])
            out[f"{name}/{tname}"] = arr if raw else np.array(_digest(arr))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    return path


@pytest.fixture(scope="module")
def golden():
    assert os.path.exists(GOLDEN), f"golden file missing: {GOLDEN}"
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", _NAMES)
def test_fa_wg_order_vs_reference(name):
    """Bounds of test_fa_forward (out 2.5e-2, lse 1e-2 absolute) and
    test_fa_backward (max error over max magnitude < 4e-2), over every row:
    the outputs come from torch.empty inside the op, so a tile that no
    workgroup took holds stale memory and a NaN or a wrong row fails here."""
    ro, rlse, rdq, rdk, rdv, vis = _reference(name)
    got = _runs(name)[0]
    b, sq, sk, h, hk, d = _CASES[name][:6]
    o = got["out"].float()
    lse = got["lse"]
    assert o.shape == ro.shape and lse.shape == rlse.shape
    vis_o = vis.view(b, sq, 1, 1).expand_as(o)
    vis_l = vis.expand_as(lse)
    do = (o - ro.float()).abs()[vis_o]
    dl = (lse - rlse).abs()[vis_l]
    print(f"{name} out err {float(do.max()):.4g} lse err "
          f"{float(dl.max()):.4g}")
    assert do.max() < 2.5e-2, f"out err {do.max()}"
    assert dl.max() < 1e-2, f"lse err {dl.max()}"
    # rows that see no key: zero output, lse = -inf
    assert (o[~vis_o] == 0).all(), "out of a row without keys is not zero"
    assert (lse[~vis_l] == float("-inf")).all(), \
        "lse of a row without keys is not -inf"
    for tname, want in (("dq", rdq), ("dk", rdk), ("dv", rdv)):
        g = got[tname].float()
        assert g.shape == want.shape
        err = (g - want.float()).abs().max()
        base = want.float().abs().max().clamp_min(1.0)
        print(f"{name} {tname}: err/base = {float(err / base):.4g}")
        assert err / base < 4e-2, f"{tname} err {err} (max {base})"


@pytest.mark.parametrize("name", _NAMES)
def test_fa_wg_order_deterministic(name):
    first, second = _runs(name)
    for tname in _OUTS:
        assert np.array_equal(_patterns(tname, first[tname]),
                              _patterns(tname, second[tname])), \
            f"{tname} differs between two calls"


@pytest.mark.parametrize("name", _NAMES)
def test_fa_wg_order_bit_identical(golden, name):
    got = _runs(name)[0]
    for tname in _OUTS:
        arr = _patterns(tname, got[tname])
        want = golden[f"{name}/{tname}"]
        if want.dtype.kind == "i":
            assert arr.shape == want.shape, f"{tname}: shape {arr.shape}"
            ndiff = int((arr != want).sum())
            assert ndiff == 0, \
                f"{tname}: {ndiff} of {arr.size} patterns differ"
        else:
            assert _digest(arr) == str(want), \
                f"{tname}: bit patterns differ from the recorded build"
