"""GPU numerics of flash_attn_varlen_with_kvcache (the PACKED instances of
csrc/flash_attn_kvcache_mq.hip) against the padded chunk op and _ref_chunk.

One batch holds every hazard at once (N / L below): a decoding row, empty
sequences in the middle and at the end, 33 and 32 rows (one MFMA row tile and
one row more at heads (4, 4)), a second row tile holding 4 rows at heads
(8, 2), L = n and a full cache. Inputs are rounded to the kernel dtype first.

  - A sequence with more than 32 packed rows: output and lse are bitwise the
    chunk op's on the padded copy at the same num_splits.
  - A sequence with at most 32 packed rows (a decoding row, a short
    verification) is held to the bound a body of its own for such rows would
    be held to: with the error measure of test_kvcache_chunk.py
    (scale-relative out, absolute lse) against _ref_chunk in fp32,
    new <= 1.5 * old + 1e-3, old = the chunk op's error on the same sequence.
    The kernel as it stands runs these rows through the same body, so old and
    new agree to every digit.

Measured on an MI355X (largest value over those sequences, every case and
both num_splits; old = padded chunk op, new = packed op):
    dtype  out old   out new   lse old   lse new
    bf16   3.26e-3   3.26e-3   9.5e-7    9.5e-7
    fp16   6.02e-4   6.02e-4   9.5e-7    9.5e-7
"""
import math

import pytest
import torch

from tests.ops.test_kvcache_chunk import (_errs, _i32, _paginate, _quant,
                                          _scales)

pytestmark = pytest.mark.gpu

BF16, FP16 = torch.bfloat16, torch.float16
CAP = 512
N = [1, 0, 33, 5, 32, 64, 0]
L = [300, 17, 257, 5, 512, 64, 0]


def _ops():
    from torchacc_amd.ops import (flash_attn_chunk_with_kvcache,
                                  flash_attn_varlen_with_kvcache)
    return flash_attn_varlen_with_kvcache, flash_attn_chunk_with_kvcache


def _batch(n, heads, d, dtype, layout, seed=0):
    """-> (packed q, padded q, k, v on the GPU, kwargs, fp32 CPU q_pad, k, v
    as the kernels see them)."""
    from torchacc_amd.ops.flash_attn import dequantize_kv_fp8
    hq, hk = heads
    b, T, sq = len(n), sum(n), max(max(n), 1)
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(T, hq, d, generator=g).to(dtype).float()
    k = torch.randn(b, CAP, hk, d, generator=g).to(dtype).float()
    v = torch.randn(b, CAP, hk, d, generator=g).to(dtype).float()
    qpad = torch.zeros(b, sq, hq, d)
    t = 0
    for i, ni in enumerate(n):
        qpad[i, :ni] = q[t:t + ni]
        t += ni
    kw = {}
    if layout == "fp8":
        ks, vs = _scales(hk, seed)
        gk, gv = _quant(k, ks).cuda(), _quant(v, vs).cuda()
        k, v = dequantize_kv_fp8(gk.cpu(), ks), dequantize_kv_fp8(gv.cpu(), vs)
        kw = {"k_scale": ks.cuda(), "v_scale": vs.cuda()}
    else:
        gk, gv = k.to("cuda", dtype), v.to("cuda", dtype)
    return q.to("cuda", dtype), qpad.to("cuda", dtype), gk, gv, kw, qpad, k, v


def _cu(n):
    return _i32([0] + torch.tensor(n).cumsum(0).tolist()).cuda()


def _compare(n, lens, heads, d, dtype, layout, wl=-1, poison=False, seed=0):
    from torchacc_amd.ops.flash_attn import _gather_pages, _ref_chunk
    varlen, chunk = _ops()
    rep = heads[0] // heads[1]
    q, qpad, gk, gv, kw, cq, ck, cv = _batch(n, heads, d, dtype, layout, seed)
    glens, gn, cu = _i32(lens).cuda(), _i32(n).cuda(), _cu(n)
    ref, ref_lse = _ref_chunk(cq, ck, cv, _i32(lens), _i32(n),
                              1.0 / math.sqrt(d), wl)
    if poison:      # every slot at or past L (no window: all others are seen)
        for i, li in enumerate(lens):
            gk[i, li:] = float("nan")
            gv[i, li:] = float("nan")
    pk, pv, pkw = gk, gv, dict(kw)
    if layout == "paged16":
        pk, pv, table, _ = _paginate(gk, gv, 16, seed=seed)
        pkw["block_table"] = table
    worst = [0.0] * 4
    for ns in (1, 3):
        out, lse = varlen(q, pk, pv, glens, cu, window_size=(wl, -1),
                          return_lse=True, num_splits=ns, **pkw)
        assert out.shape == q.shape and lse.shape == (heads[0], sum(n))
        assert out.dtype == dtype and lse.dtype == torch.float32
        if layout == "paged16":     # bitwise the contiguous, gathered cache
            same = varlen(q, _gather_pages(pk, table), _gather_pages(pv, table),
                          glens, cu, window_size=(wl, -1), return_lse=True,
                          num_splits=ns, **kw)
            assert torch.equal(out, same[0]) and torch.equal(lse, same[1])
        pad, pad_lse = chunk(qpad, gk, gv, glens, q_seqlens=gn,
                             window_size=(wl, -1), return_lse=True,
                             num_splits=ns, **kw)
        t = 0
        for i, ni in enumerate(n):
            if ni == 0:
                continue
            o_i, l_i = out[t:t + ni], lse[:, t:t + ni]
            if ni * rep > 32:
                assert torch.equal(o_i, pad[i, :ni]), (i, ns)
                assert torch.equal(l_i, pad_lse[i, :, :ni]), (i, ns)
            r_i, rl_i = ref[i, :ni], ref_lse[i, :, :ni]
            no, nl = _errs(o_i, l_i, r_i, rl_i)
            oo, ol = _errs(pad[i, :ni], pad_lse[i, :, :ni], r_i, rl_i)
            if ni * rep <= 32:
                worst = [max(a, b) for a, b in zip(worst, (oo, no, ol, nl))]
                assert no <= 1.5 * oo + 1e-3, (i, ns, no, oo)
                assert nl <= 1.5 * ol + 1e-3, (i, ns, nl, ol)
            t += ni
    print(f"short {dtype} d{d} {heads} {layout} n{n} wl{wl}: out old "
          f"{worst[0]:.3e} new {worst[1]:.3e}  lse old {worst[2]:.3e} new "
          f"{worst[3]:.3e}")
    return out, lse


@pytest.mark.parametrize("layout", ["contiguous", "paged16", "fp8"])
@pytest.mark.parametrize("heads", [(8, 2), (4, 4), (32, 2)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", [BF16, FP16])
def test_hazard_batch(dtype, d, heads, layout):
    _compare(N, L, heads, d, dtype, layout)


@pytest.mark.parametrize("heads", [(8, 2), (4, 4)])
def test_fewer_keys_than_rows_window_and_poison(heads):
    """L < n (rows with p < 0 are zero rows, lse = -inf: _errs checks the
    -inf pattern), a left window of 40, and NaN in every invisible slot."""
    out, lse = _compare([5, 33], [3, 20], heads, 128, BF16, "contiguous")
    assert bool((out[:2] == 0).all()) and bool(torch.isinf(lse[:, :2]).all())
    _compare(N, L, heads, 128, BF16, "paged16", wl=40)
    clean = _compare(N, L, heads, 64, FP16, "contiguous", seed=3)
    dirty = _compare(N, L, heads, 64, FP16, "contiguous", seed=3, poison=True)
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1])


def test_graph_capture_follows_lengths_and_cu():
    varlen, _ = _ops()
    n = [1, 40, 5]
    q, _, gk, gv, _, _, _, _ = _batch(n, (8, 2), 128, BF16, "contiguous", 4)
    lens, cu = _i32([300, 512, 64]).cuda(), _cu(n)

    def call():
        return varlen(q, gk, gv, lens, cu, return_lse=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = call()
    for new_lens, new_n in (([300, 512, 64], n), ([40, 41, 512], [6, 0, 40]),
                            ([7, 100, 3], [20, 20, 6])):
        lens.copy_(_i32(new_lens))
        cu.copy_(_cu(new_n))
        for _ in range(2):
            graph.replay()
        eager, eager_lse = call()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(lse, eager_lse)
