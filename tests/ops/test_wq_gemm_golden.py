"""The weight-only quantised GEMMs (fp8_linear.hip, mxfp4_linear.hip) must stay
bit-identical to the build that still had eight kernel templates and five
separate host front ends: y as 16-bit patterns, at the smallest shapes that
reach every instance and every edge (row clamp, channel clamp, N % 4 != 0,
K below one step, ragged last step, several steps per wave slot, capped and
uncapped splits), in bf16 and fp16, with and without bias.

The bound _C names are called directly and every choice that depends on the
CU count (num_splits, waves, tiles) is forced, so the device plays no part.

A pytest case is one (op, dtype, bias) group and loops over its shapes. The
golden file holds, per group, the SHA-256 over every result of the group in
order, and the leading 64 bits of each result's own SHA-256, which name the
shape that differs. record_golden() below wrote it (run by hand on the
earlier build, see profiles/r21_wq_gemm_refactor.md)."""
import functools
import hashlib
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                      "golden", "wq_gemm.npz")
_DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
FP8 = torch.float8_e4m3fn
# masters that every case slices: rows, channels, K
_MAX_M, _MAX_N, _MAX_K = 129, 130, 2080


@functools.lru_cache(maxsize=None)
def _masters(dt):
    """CPU masters, generated once per dtype from a fixed seed and never
    modified: x, two e4m3 weights with scales, two MXFP4 weights (codes, scale
    bytes), two biases."""
    g = torch.Generator().manual_seed(4321 + (dt == "fp16"))
    dtype = _DT[dt]
    # fp16: small activations, so that the largest MXFP4 scales (2^12) and the
    # SwiGLU product leave most results finite
    x = (torch.randn(_MAX_M, _MAX_K, generator=g) *
         (2.0 ** -8 if dt == "fp16" else 1.0)).to(dtype)
    w8 = [(torch.randn(_MAX_N, _MAX_K, generator=g) * 60).clamp(-448, 448)
          .to(FP8) for _ in range(2)]
    s8 = [torch.rand(_MAX_N, generator=g) * 0.02 + 0.001 for _ in range(2)]
    codes = [torch.randint(0, 256, (_MAX_N, _MAX_K // 2), generator=g,
                           dtype=torch.uint8) for _ in range(2)]
    shape = (_MAX_N, _MAX_K // 32)
    if dt == "fp16":
        # the fp16 contract, exponents -14..12 (bytes 113..139), mostly low
        sb = [(113 + (27 * torch.rand(shape, generator=g) ** 4).floor())
              .clamp(113, 139).to(torch.uint8) for _ in range(2)]
    else:
        sb = [torch.randint(70, 176, shape, generator=g, dtype=torch.uint8)
              for _ in range(2)]
        # bytes 0 and 1 (the clamp) in the first groups, where every K sees them
        for s in sb:
            s[0::5, 0] = 0
            s[1::5, 0] = 1
            s[2::7, 1] = 0
    bias = [torch.randn(_MAX_N, generator=g).to(dtype) for _ in range(2)]
    return x, w8, s8, codes, sb, bias


@functools.lru_cache(maxsize=None)
def _x(dt, m, k):
    return _masters(dt)[0][:m, :k].contiguous().cuda()


@functools.lru_cache(maxsize=None)
def _w8(dt, which, n, k):
    _, w8, s8, _, _, _ = _masters(dt)
    w = w8[which].view(torch.uint8)[:n, :k].contiguous().view(FP8)
    return w.cuda(), s8[which][:n].contiguous().cuda()


@functools.lru_cache(maxsize=None)
def _w4(dt, which, n, k):
    _, _, _, codes, sb, _ = _masters(dt)
    return (codes[which][:n, :k // 2].contiguous().cuda(),
            sb[which][:n, :k // 32].contiguous().cuda())


@functools.lru_cache(maxsize=None)
def _bias(dt, which, n):
    return _masters(dt)[5][which][:n].contiguous().cuda()


def _b(dt, which, n, on):
    return _bias(dt, which, n) if on else None


def _ext():
    from torchacc_amd.ops._backend import require_extension
    return require_extension()


# ---- the shapes of each op --------------------------------------------------
# fp8 skinny instances (waves, tiles) per K: 8 waves need 8 steps of 128 codes
_FP8_INST = {144: ((4, 1), (4, 2)), 1040: ((4, 1), (8, 1), (4, 2), (8, 2))}
_FP8_SW_WAVES = {144: (4,), 1040: (4, 8)}
# MXFP4 skinny instances per K: 8 waves need 8 steps of 256 codes
_MX4_W4 = ((4, 1), (4, 2), (4, 4))
_MX4_INST = {32: _MX4_W4, 256: _MX4_W4, 288: _MX4_W4,
             2080: ((4, 1), (8, 1), (4, 2), (8, 2), (4, 4))}
_MX4_SW_INST = {288: ((4, 2), (4, 4)), 2080: ((4, 2), (8, 2), (4, 4))}
_SKINNY_M = (1, 17, 33)
_TILED_M = (65, 129)
_SPLITS = (1, 2, 16)


def _shapes_fp8_linear():
    return itertools.product((1, 17, 64, 70), (32, 40, 30),
                             (16, 128, 144, 1040), (1, 3, 16))


def _shapes_fp8_linear_wide():
    for k, insts in _FP8_INST.items():
        for (w, nt), m, n in itertools.product(insts, _SKINNY_M, (16, 30, 40)):
            yield m, n, k, w, nt


def _shapes_fp8_swiglu_linear():
    for k, waves in _FP8_SW_WAVES.items():
        yield from itertools.product(_SKINNY_M, (16, 30), (k,), waves)


def _shapes_fp8_gemm():
    return itertools.product(_TILED_M, (128, 130), (48, 64, 80, 272), _SPLITS)


def _shapes_mxfp4_linear():
    for k, insts in _MX4_INST.items():
        for (w, nt), m, n in itertools.product(insts, _SKINNY_M, (16, 30, 70)):
            yield m, n, k, w, nt


def _shapes_mxfp4_swiglu_linear():
    for k, insts in _MX4_SW_INST.items():
        for (w, nt), m, n in itertools.product(insts, _SKINNY_M, (16, 30)):
            yield m, n, k, w, nt


def _shapes_mxfp4_gemm():
    return itertools.product(_TILED_M, (64, 70, 130), (32, 64, 96, 288),
                             _SPLITS)


# bias modes: plain ops take 0 / 1, the SwiGLU ops (gate, up) pairs
_PLAIN_BIAS = {"nobias": (False,), "bias": (True,)}
_PAIR_BIAS = {"nobias": (False, False), "gate": (True, False),
              "both": (True, True)}


def _run(op, dt, bias, shape):
    """One call of a bound name; returns y."""
    ext = _ext()
    if op == "fp8_linear" or op == "fp8_gemm":
        m, n, k, ns = shape
        w, s = _w8(dt, 0, n, k)
        return getattr(ext, op)(_x(dt, m, k), w, s, _b(dt, 0, n, bias[0]), ns)
    if op == "fp8_linear_wide":
        m, n, k, waves, tiles = shape
        w, s = _w8(dt, 0, n, k)
        return ext.fp8_linear_wide(_x(dt, m, k), w, s, _b(dt, 0, n, bias[0]),
                                   waves, tiles)
    if op == "fp8_swiglu_linear":
        m, n, k, waves = shape
        wg, sg = _w8(dt, 0, n, k)
        wu, su = _w8(dt, 1, n, k)
        return ext.fp8_swiglu_linear(_x(dt, m, k), wg, sg, wu, su,
                                     _b(dt, 0, n, bias[0]),
                                     _b(dt, 1, n, bias[1]), waves)
    if op == "mxfp4_linear":
        m, n, k, waves, tiles = shape
        c, s = _w4(dt, 0, n, k)
        return ext.mxfp4_linear(_x(dt, m, k), c, s, _b(dt, 0, n, bias[0]),
                                waves, tiles)
    if op == "mxfp4_gemm":
        m, n, k, ns = shape
        c, s = _w4(dt, 0, n, k)
        return ext.mxfp4_gemm(_x(dt, m, k), c, s, _b(dt, 0, n, bias[0]), ns)
    cg, sg = _w4(dt, 0, shape[1], shape[2])
    cu, su = _w4(dt, 1, shape[1], shape[2])
    m, n, k = shape[:3]
    bg, bu = _b(dt, 0, n, bias[0]), _b(dt, 1, n, bias[1])
    if op == "mxfp4_swiglu_linear":
        return ext.mxfp4_swiglu_linear(_x(dt, m, k), cg, sg, cu, su, bg, bu,
                                       shape[3], shape[4])
    assert op == "mxfp4_swiglu_gemm"
    return ext.mxfp4_swiglu_gemm(_x(dt, m, k), cg, sg, cu, su, bg, bu,
                                 shape[3])


# op: (shape generator, bias modes)
_OPS = {
    "fp8_linear": (_shapes_fp8_linear, _PLAIN_BIAS),
    "fp8_linear_wide": (_shapes_fp8_linear_wide, _PLAIN_BIAS),
    "fp8_swiglu_linear": (_shapes_fp8_swiglu_linear, _PAIR_BIAS),
    "fp8_gemm": (_shapes_fp8_gemm, _PLAIN_BIAS),
    "mxfp4_linear": (_shapes_mxfp4_linear, _PLAIN_BIAS),
    "mxfp4_swiglu_linear": (_shapes_mxfp4_swiglu_linear, _PAIR_BIAS),
    "mxfp4_gemm": (_shapes_mxfp4_gemm, _PLAIN_BIAS),
    "mxfp4_swiglu_gemm": (_shapes_mxfp4_gemm, _PAIR_BIAS),
}
_GROUPS = [(op, dt, bm) for op in _OPS for dt in _DT for bm in _OPS[op][1]]


def _bits(y, dt, shape):
    assert y.dtype == _DT[dt] and tuple(y.shape) == tuple(shape), \
        (y.dtype, y.shape)
    return y.cpu().contiguous().view(torch.int16).numpy().tobytes()


def _run_group(op, dt, bm):
    """(shapes, leading 64 bits of each result's SHA-256, SHA-256 of all)."""
    gen, modes = _OPS[op]
    shapes = list(gen())
    ys = [_run(op, dt, modes[bm], s) for s in shapes]   # one sync at the end
    whole = hashlib.sha256()
    heads = np.empty(len(shapes), dtype=np.uint64)
    for i, (s, y) in enumerate(zip(shapes, ys)):
        b = _bits(y, dt, s[:2])
        whole.update(b)
        heads[i] = int.from_bytes(hashlib.sha256(b).digest()[:8], "little")
    return shapes, heads, whole.hexdigest()


def _run_dequantize(dt):
    c, s = _w4(dt, 0, 5, 96)
    return _bits(_ext().mxfp4_dequantize(c, s, _DT[dt]), dt, (5, 96))


def record_golden(path=GOLDEN):
    """Run by hand on the build whose results are to be kept:
    python -c "from tests.ops.test_wq_gemm_golden import record_golden
    as r; r()" """
    out = {}
    for op, dt, bm in _GROUPS:
        _, heads, whole = _run_group(op, dt, bm)
        out[f"{op}/{dt}/{bm}/heads"] = heads
        out[f"{op}/{dt}/{bm}/sha256"] = np.array(whole)
    for dt in _DT:
        out[f"mxfp4_dequantize/{dt}"] = np.frombuffer(_run_dequantize(dt),
                                                      dtype=np.int16)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    return path


@pytest.fixture(scope="module")
def golden():
    assert os.path.exists(GOLDEN), f"golden file missing: {GOLDEN}"
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("op,dt,bm", _GROUPS)
def test_bit_identical(golden, op, dt, bm):
    shapes, heads, whole = _run_group(op, dt, bm)
    want = golden[f"{op}/{dt}/{bm}/heads"]
    assert want.shape == heads.shape, "the golden file is for other shapes"
    bad = [shapes[i] for i in np.nonzero(want != heads)[0]]
    assert not bad, f"{op} {dt} {bm}: {len(bad)} of {len(shapes)} results " \
                    f"differ from the recorded build, first {bad[:8]}"
    assert whole == str(golden[f"{op}/{dt}/{bm}/sha256"])


@pytest.mark.parametrize("dt", sorted(_DT))
def test_dequantize_bit_identical(golden, dt):
    got = np.frombuffer(_run_dequantize(dt), dtype=np.int16)
    want = golden[f"mxfp4_dequantize/{dt}"]
    assert want.shape == got.shape
    assert int((got != want).sum()) == 0
