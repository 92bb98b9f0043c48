"""KV-cache attention (flash_attn_with_kvcache, flash_attn_chunk_with_kvcache)
must stay bit-identical to the build that still had a separate fp8 decode
kernel and eight bound entry points: `out` as 16-bit patterns, `lse` as 32-bit
patterns, at the smallest shapes that reach every instance and every edge of
the split kernel and all four variants of the multi-query kernel.

Only the public Python API is used, so the file runs on either build. Every
decode case sets num_splits, so the device's CU count plays no part.

The golden file holds what the earlier build computed; record_golden() below
wrote it (run by hand on that build, see profiles/r10_kvcache_refactor.md)."""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                      "golden", "kvcache_attn.npz")
_BF, _FP = torch.bfloat16, torch.float16
FP8 = torch.float8_e4m3fn
PAGE = 16

# ---- decode -----------------------------------------------------------------
# Lengths: 0, an empty sequence; 1, one key; 65, one key into the second
# 64-key tile (the third 32-key tile); 300, a partial last tile at both tile
# sizes, short of cap. With 3 splits the short sequences leave empty splits,
# which the combine skips, and 300 keys do not divide evenly.
DEC_CAP = 320
DEC_LENS = (0, 1, 65, 300)
DEC_SPLITS = (1, 3)
_ALL = ("contig16", "paged16", "contig8", "paged8")
# name: (hq, hk, d, dtype, left window, with cache_seqlens, variants)
_DEC_CASES = {}
for _d in (128, 64):
    # R = 1, 2, 4, 8
    for _hq in (2, 4, 8, 16):
        _DEC_CASES[f"d{_d}_h{_hq}_2"] = (_hq, 2, _d, _BF, -1, True, _ALL)
    _DEC_CASES[f"d{_d}_h8_2_fp16"] = (8, 2, _d, _FP, -1, True, _ALL)
# two row groups, the second with 4 real rows in an R = 8 instance
_DEC_CASES["d128_h12_1"] = (12, 1, 128, _BF, -1, True, _ALL)
_DEC_CASES["d128_h8_2_window40"] = (8, 2, 128, _BF, 40, True, _ALL)
# no cache_seqlens: every sequence is cap long (contiguous layout only)
_DEC_CASES["d128_h8_2_nolens"] = (8, 2, 128, _BF, -1, False,
                                  ("contig16", "contig8"))
_DEC_PARAMS = [(name, var, ns) for name in sorted(_DEC_CASES)
               for var in _DEC_CASES[name][6] for ns in DEC_SPLITS]

# ---- chunk ------------------------------------------------------------------
CH_CAP = 192
CH_SQ = 5
CH_LENS = (5, 70, 130)
CH_QLENS = (5, 3, 0)
# name: (hq, hk, d, dtype, left window)
_CH_CASES = {
    "d128_h8_2": (8, 2, 128, _BF, -1),
    "d64_h8_2": (8, 2, 64, _BF, -1),
    "d128_h8_2_window40": (8, 2, 128, _BF, 40),
}
_CH_PARAMS = [(name, var) for name in sorted(_CH_CASES) for var in _ALL]

# Raw patterns are stored for a result of at most this many elements (out and
# lse together); a larger one is stored as the SHA-256 of the same patterns.
_RAW_LIMIT = 2100


def _scales(hk):
    h = torch.arange(hk, dtype=torch.float32)
    return 0.0173 * (1.0 + 0.31 * h), 0.0119 * (1.0 + 0.23 * h)


@functools.lru_cache(maxsize=None)
def _make(b, sq, cap, hq, hk, d, dtype):
    """CPU inputs, shared between cases and never modified in place: q, the
    16-bit caches, the e4m3 caches with their scales, and one page table."""
    g = torch.Generator().manual_seed(1234)
    q = torch.randn(b, sq, hq, d, generator=g).to(dtype)
    k = torch.randn(b, cap, hk, d, generator=g)
    v = torch.randn(b, cap, hk, d, generator=g)
    ks, vs = _scales(hk)
    k8 = (k / ks.view(1, 1, -1, 1)).clamp(-448, 448).to(FP8)
    v8 = (v / vs.view(1, 1, -1, 1)).clamp(-448, 448).to(FP8)
    w = cap // PAGE
    assert w * PAGE == cap
    # two spare pages that no table entry names
    perm = torch.randperm(b * w + 2, generator=g)
    table = perm[:b * w].view(b, w).to(torch.int32)
    return q, k.to(dtype), v.to(dtype), k8, v8, ks, vs, table


def _paginate(c, table):
    """contiguous [b, cap, hk, d] -> pool [b * w + 2, PAGE, hk, d] (zeros in
    the spare pages) in which table[i, j] holds page j of sequence i."""
    b, cap, hk, d = c.shape
    n = table.numel() + 2
    raw = c.view(torch.uint8) if c.dtype == FP8 else c
    pool = torch.zeros(n, PAGE, hk, d, dtype=raw.dtype)
    pool[table.reshape(-1).long()] = raw.reshape(-1, PAGE, hk, d)
    return pool.view(FP8) if c.dtype == FP8 else pool


def _cache_kwargs(inputs, variant):
    """(k_cache, v_cache, kwargs) on the GPU for one of the four variants."""
    _, k, v, k8, v8, ks, vs, table = inputs
    kw = {}
    if variant.endswith("8"):
        k, v = k8, v8
        kw.update(k_scale=ks.cuda(), v_scale=vs.cuda())
    if variant.startswith("paged"):
        k, v = _paginate(k, table), _paginate(v, table)
        kw.update(block_table=table.cuda())
    return k.cuda(), v.cuda(), kw


def _bits(out, lse):
    assert out.dtype in (_BF, _FP) and lse.dtype == torch.float32
    return (out.cpu().contiguous().view(torch.int16).numpy(),
            lse.cpu().contiguous().view(torch.int32).numpy())


def _run_decode(name, variant, ns):
    from torchacc_amd.ops import flash_attn_with_kvcache
    hq, hk, d, dtype, wl, with_lens, _ = _DEC_CASES[name]
    inputs = _make(len(DEC_LENS), 1, DEC_CAP, hq, hk, d, dtype)
    k, v, kw = _cache_kwargs(inputs, variant)
    if with_lens:
        kw.update(cache_seqlens=torch.tensor(DEC_LENS, dtype=torch.int32,
                                             device="cuda"))
    out, lse = flash_attn_with_kvcache(
        inputs[0].cuda(), k, v, window_size=(wl, -1), num_splits=ns,
        return_lse=True, **kw)
    return _bits(out, lse)


def _run_chunk(name, variant):
    from torchacc_amd.ops import flash_attn_chunk_with_kvcache
    hq, hk, d, dtype, wl = _CH_CASES[name]
    inputs = _make(len(CH_LENS), CH_SQ, CH_CAP, hq, hk, d, dtype)
    k, v, kw = _cache_kwargs(inputs, variant)
    out, lse = flash_attn_chunk_with_kvcache(
        inputs[0].cuda(), k, v,
        torch.tensor(CH_LENS, dtype=torch.int32, device="cuda"),
        q_seqlens=torch.tensor(CH_QLENS, dtype=torch.int32, device="cuda"),
        window_size=(wl, -1), return_lse=True, **kw)
    return _bits(out, lse)


def _digest(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


def record_golden(path=GOLDEN):
    """Run by hand on the build whose results are to be kept:
    python -c "from tests.ops.test_kvcache_attn_golden import record_golden
    as r; r()" """
    out = {}
    runs = [(f"decode/{n}/{var}/ns={ns}", _run_decode(n, var, ns))
            for n, var, ns in _DEC_PARAMS]
    runs += [(f"chunk/{n}/{var}", _run_chunk(n, var)) for n, var in _CH_PARAMS]
    for key, arrs in runs:
        raw = sum(a.size for a in arrs) <= _RAW_LIMIT
        for tname, arr in zip(("out", "lse"), arrs):
            out[f"{key}/{tname}"] = arr if raw else np.array(_digest(arr))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    return path


@pytest.fixture(scope="module")
def golden():
    assert os.path.exists(GOLDEN), f"golden file missing: {GOLDEN}"
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _compare(golden, key, arrs):
    for tname, arr in zip(("out", "lse"), arrs):
        want = golden[f"{key}/{tname}"]
        if want.dtype.kind == "i":
            assert want.dtype == arr.dtype and want.shape == arr.shape
            ndiff = int((arr != want).sum())
            assert ndiff == 0, \
                f"{key} {tname}: {ndiff} of {arr.size} patterns differ"
        else:
            assert _digest(arr) == str(want), \
                f"{key} {tname}: bit patterns differ from the recorded build"


@pytest.mark.parametrize("name,variant,ns", _DEC_PARAMS)
def test_decode_bit_identical(golden, name, variant, ns):
    _compare(golden, f"decode/{name}/{variant}/ns={ns}",
             _run_decode(name, variant, ns))


@pytest.mark.parametrize("name,variant", _CH_PARAMS)
def test_chunk_bit_identical(golden, name, variant):
    _compare(golden, f"chunk/{name}/{variant}", _run_chunk(name, variant))
