"""GPU numerics of flash_attn_chunk_with_kvcache (csrc/flash_attn_kvcache_mq.hip).

Inputs are rounded to the kernel dtype BEFORE the fp32 reference (_ref_chunk,
the op's CPU path) is computed, so the error measured is the kernel's own.

Error measure. out: max|got - ref| / max|ref| over the whole tensor; lse:
max|got - ref| over the rows that see a key. The output error is taken
relative to the output scale because both kernels round P and the output to
16 bits, which gives errors proportional to the magnitude of the output, and
that magnitude depends on how many keys a row sees (one key: |out| = |v| up
to ~4; 512 keys: ~0.2). Absolute errors of cases with different context
lengths are therefore not comparable, scale-relative ones are.

Bound. The new kernel rounds P to 16 bits before PV, as fa_fwd_kernel does,
so it is measured against that kernel. On the cases both can express
(contiguous, every L = cap, every n = sq) the test computes the error of
``fa_forward`` and of the new op against the same fp32 reference and requires
    new <= 1.5 * old + 1e-3                       (out and lse alike)
per case; the factor allows for another tile order, not another algorithm.
For a case fa_forward cannot express, ``old`` in that formula is the largest
error fa_forward reaches over the expressible cases of the same dtype and
head dim (EXPRESSIBLE below).

Measured on an MI355X (old = fa_forward, largest value over the expressible
cases; "grid" = largest error of the new op over every other case here):
    dtype d    out old   out new   out bound  grid out   lse old/new  lse bound  grid lse
    bf16  64   4.62e-3   4.62e-3   7.93e-3    3.48e-3    9.5e-7       1.0e-3     1.4e-6
    bf16  128  3.60e-3   3.60e-3   6.40e-3    3.33e-3    9.5e-7       1.0e-3     1.4e-6
    fp16  64   5.62e-4   5.62e-4   1.84e-3    5.88e-4    9.5e-7       1.0e-3     1.4e-6
    fp16  128  5.29e-4   5.29e-4   1.79e-3    4.73e-4    9.5e-7       1.0e-3     1.4e-6
On the expressible cases old and new agree to every printed digit: the tile
order and the arithmetic are fa_fwd_kernel's.

What the bound separates (CPU emulation at these shapes: cap 512, d 64 and
128, bf16 inputs, heads (8, 2), (32, 2), (4, 4), fp32 arithmetic, (L, n) in
(512, 200), (512, 1), (512, 17), (257, 64)): making ONE visible key
invisible to every row changes the scale-relative output by 0.012 .. 0.56
and some row's lse by 0.003 .. 0.16. The cheapest key to lose is the last one
(L - 1): only the last query position sees it. Keys L / 2 and L - n, which
every row sees, cost >= 0.036 / 0.004. The bounds are <= 0.008 for out and
1.0e-3 for lse, so a single lost or extra key fails; shorter contexts only
raise the cost of a key.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, FP16, FP8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
CAP = 512
# decode tests' bounds, for the n = 1 rows compared with the decode op
OUT_REL = 1.5e-2
LSE_ABS = 1e-2
HEADS = [(8, 2), (4, 4), (28, 4), (32, 2)]
SQS = [1, 3, 17, 64, 200]


def _ops():
    from torchacc_amd.ops import (flash_attn_chunk_with_kvcache,
                                  flash_attn_with_kvcache)
    return flash_attn_chunk_with_kvcache, flash_attn_with_kvcache


def _fn():
    return _ops()[0]


def _make(b, sq, hq, hk, d, dtype, seed=0, cap=CAP):
    """CPU tensors already rounded to `dtype`, held in fp32."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, sq, hq, d, generator=g).to(dtype).float()
    k = torch.randn(b, cap, hk, d, generator=g).to(dtype).float()
    v = torch.randn(b, cap, hk, d, generator=g).to(dtype).float()
    return q, k, v


def _gpu(t, dtype):
    return t.to("cuda", dtype)


def _i32(vals):
    return torch.tensor(vals, dtype=torch.int32)


def _errs(out, lse, ref, ref_lse):
    """(scale-relative out error, lse error); also checks the empty rows."""
    out, lse = out.float().cpu(), lse.float().cpu()
    assert out.shape == ref.shape and lse.shape == ref_lse.shape
    assert bool(torch.isfinite(out).all()), "non-finite output"
    empty = torch.isinf(ref_lse)
    assert torch.equal(torch.isinf(lse) & (lse < 0), empty), \
        "lse = -inf rows differ"
    scale = float(ref.abs().max())
    err = float((out - ref).abs().max())
    oerr = err / scale if scale > 0 else err
    lerr = 0.0
    if bool((~empty).any()):
        lerr = float((lse - ref_lse)[~empty].abs().max())
    return oerr, lerr


# ---- the yardstick: fa_forward on the cases both kernels can express ---------
EXPRESSIBLE = list(zip(SQS, HEADS + HEADS[:1]))     # (sq, heads), b = 2


@functools.lru_cache(maxsize=None)
def _baseline(dtype, d):
    """Per expressible case: (tag, old_out, old_lse, new_out, new_lse)."""
    from torchacc_amd.ops._backend import require_extension
    from torchacc_amd.ops.flash_attn import _ref_chunk
    ext = require_extension()
    fn = _fn()
    rows = []
    e = torch.empty(0)
    for sq, (hq, hk) in EXPRESSIBLE:
        q, k, v = _make(2, sq, hq, hk, d, dtype, seed=sq)
        lens = _i32([CAP, CAP])
        scale = 1.0 / math.sqrt(d)
        ref, ref_lse = _ref_chunk(q, k, v, lens, None, scale, -1)
        gq, gk, gv = (_gpu(t, dtype) for t in (q, k, v))
        old = ext.fa_forward(gq, gk, gv, scale, True, -1, -1, e, e, e, 0.0, 0)
        new = fn(gq, gk, gv, lens.cuda(), return_lse=True)
        oo, ol = _errs(old[0], old[1], ref, ref_lse)
        no, nl = _errs(new[0], new[1], ref, ref_lse)
        tag = f"{dtype} d{d} sq{sq} heads{(hq, hk)}"
        print(f"expressible {tag}: out old {oo:.3e} new {no:.3e}  "
              f"lse old {ol:.3e} new {nl:.3e}")
        rows.append((tag, oo, ol, no, nl))
    return rows


def _bounds(dtype, d):
    rows = _baseline(dtype, d)
    return (1.5 * max(r[1] for r in rows) + 1e-3,
            1.5 * max(r[2] for r in rows) + 1e-3)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", [BF16, FP16])
def test_expressible_cases_against_fa_forward(dtype, d):
    for tag, oo, ol, no, nl in _baseline(dtype, d):
        assert no <= 1.5 * oo + 1e-3, (tag, no, oo)
        assert nl <= 1.5 * ol + 1e-3, (tag, nl, ol)


def _check(out, lse, ref, ref_lse, dtype, d, tag):
    oerr, lerr = _errs(out, lse, ref, ref_lse)
    ob, lb = _bounds(dtype, d)
    print(f"{tag}: out err {oerr:.3e} (bound {ob:.3e})  "
          f"lse err {lerr:.3e} (bound {lb:.3e})")
    assert oerr <= ob, (tag, oerr, ob)
    assert lerr <= lb, (tag, lerr, lb)


# ---- layouts ----------------------------------------------------------------
def _paginate(k, v, ps, seed=0, extra=3, share=False, strided=False):
    """GPU pools holding the pages of k / v [b, cap, hk, d] at permuted
    physical indices (plus `extra` pages no table entry names), and the
    table. share: the first page of every sequence is ONE physical page
    (k / v must agree there). strided: the pools are every second slot of a
    larger buffer."""
    b, cap, hk, d = k.shape
    w = cap // ps
    n = b * w + extra
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    table = perm[:b * w].view(b, w).clone()
    if share:
        table[1:, 0] = table[0, 0]
    shape = (n, 2 * ps, hk, d) if strided else (n, ps, hk, d)
    kp = torch.zeros(shape, dtype=k.dtype, device=k.device)
    vp = torch.zeros(shape, dtype=k.dtype, device=k.device)
    if strided:
        kp, vp = kp[:, ::2], vp[:, ::2]
    idx = table.reshape(-1).to(k.device)
    if k.dtype == FP8:
        kp.view(torch.uint8)[idx] = k.reshape(b * w, ps, hk, d).view(torch.uint8)
        vp.view(torch.uint8)[idx] = v.reshape(b * w, ps, hk, d).view(torch.uint8)
    else:
        kp[idx] = k.reshape(b * w, ps, hk, d)
        vp[idx] = v.reshape(b * w, ps, hk, d)
    unused = perm[b * w:]
    return kp, vp, table.to(torch.int32).to(k.device), unused


def _quant(x, scale):
    y = x * (1.0 / scale).view(1, 1, -1, 1)
    return y.clamp(-448.0, 448.0).to(FP8)


def _scales(hk, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.01 + 0.02 * torch.rand(hk, generator=g),
            0.01 + 0.02 * torch.rand(hk, generator=g))


def _visible_union(L, n, sq, wl, cap=CAP):
    """[lo, hi) of the slots some row of the sequence sees."""
    L, n = min(max(L, 0), cap), min(max(n, 0), sq)
    first = max(0, n - L)                 # first row with p >= 0
    if first >= n:
        return 0, 0
    p0 = L - n + first
    return (max(0, p0 - wl) if wl >= 0 else 0), L


def _run_case(lens, sq, heads, d, dtype, qlens=None, wl=-1, ps=None,
              fp8=False, poison=False, seed=0):
    """One case on the GPU against _ref_chunk on the CPU; returns (out, lse)."""
    from torchacc_amd.ops.flash_attn import _ref_chunk, dequantize_kv_fp8
    fn = _fn()
    hq, hk = heads
    b = len(lens)
    q, k, v = _make(b, sq, hq, hk, d, dtype, seed=seed)
    scale = 1.0 / math.sqrt(d)
    ql = None if qlens is None else _i32(qlens)
    kw = {}
    if fp8:
        ks, vs = _scales(hk, seed)
        k8, v8 = _quant(k, ks), _quant(v, vs)
        k, v = dequantize_kv_fp8(k8, ks), dequantize_kv_fp8(v8, vs)
        kw = {"k_scale": ks.cuda(), "v_scale": vs.cuda()}
    ref, ref_lse = _ref_chunk(q, k, v, _i32(lens), ql, scale, wl)
    gk, gv = (k8.cuda(), v8.cuda()) if fp8 else (_gpu(k, dtype),
                                                 _gpu(v, dtype))
    if poison:
        nan = 0x7f if fp8 else float("nan")       # 0x7f is NaN in e4m3fn
        for i in range(b):
            lo, hi = _visible_union(lens[i], sq if qlens is None
                                    else qlens[i], sq, wl)
            for t in (gk, gv):
                t = t.view(torch.uint8) if fp8 else t
                t[i, hi:] = nan
                t[i, :lo] = nan
    if ps is not None:
        gk, gv, table, unused = _paginate(gk, gv, ps, seed=seed)
        kw["block_table"] = table
        if poison:
            for t in (gk, gv):
                t = t.view(torch.uint8) if fp8 else t
                t[unused.cuda()] = 0x7f if fp8 else float("nan")
            for i in range(b):   # entries past the live pages: out of range
                live = -(-min(max(lens[i], 0), CAP) // ps)
                table[i, live:] = 2 ** 30 if i % 2 else -7
    out, lse = fn(_gpu(q, dtype), gk, gv, _i32(lens).cuda(),
                  q_seqlens=None if ql is None else ql.cuda(),
                  window_size=(wl, -1), return_lse=True, **kw)
    assert out.dtype == dtype and lse.dtype == torch.float32
    assert out.shape == (b, sq, hq, d) and lse.shape == (b, hq, sq)
    _check(out, lse, ref, ref_lse, dtype, d,
           f"L{lens} n{qlens} sq{sq} {heads} d{d} {dtype} wl{wl} ps{ps} "
           f"fp8={fp8} poison={poison}")
    return out, lse


def _length_sets(sq):
    return [
        [sq, sq],                                    # empty prefix
        [63, 64, 65],
        [128, 257, 512],
        [min(sq + 63, CAP), min(sq + 64, CAP), min(sq + 65, CAP)],
        [0, sq - 1, 512],                            # L = 0, L < n
    ]


def _grid():
    """Every sq with every length set; heads, head dim, dtype and layout
    cycle so that each value meets each sq at least once."""
    cases, i = [], 0
    for sq in SQS:
        for lens in _length_sets(sq):
            heads = HEADS[i % 4]
            d = (64, 128)[(i // 2) % 2]
            dtype = (BF16, FP16)[(i // 3) % 2]
            ps = (None, 16, 64)[i % 3]
            cases.append((lens, sq, heads, d, dtype, ps))
            i += 1
    # rep 16 with sq 200 spans 25 row tiles; every heads pair at both dims
    cases += [([257, 512, 200], 200, (32, 2), 128, BF16, None),
              ([257, 512, 200], 200, (32, 2), 64, FP16, 16),
              ([65, 300], 64, (28, 4), 128, BF16, 64),
              ([65, 300], 17, (4, 4), 128, FP16, None),
              ([65, 300], 17, (8, 2), 64, BF16, 16)]
    return cases


@pytest.mark.parametrize("lens,sq,heads,d,dtype,ps", _grid())
def test_parity_grid(lens, sq, heads, d, dtype, ps):
    _run_case(lens, sq, heads, d, dtype, ps=ps)


@pytest.mark.parametrize("wl", [0, 16, 100])
@pytest.mark.parametrize("sq,heads,ps", [(17, (8, 2), None), (200, (28, 4), 16),
                                         (3, (32, 2), 64)])
def test_window(wl, sq, heads, ps):
    lens = [65, 300, 512]
    out, _ = _run_case(lens, sq, heads, 128, BF16, wl=wl, ps=ps)
    if wl == 0:
        # one visible key: p = 1, the row is V's row at its position, exactly
        hq, hk = heads
        _, _, v = _make(3, sq, hq, hk, 128, BF16)
        for i, L in enumerate(lens):
            for j in range(max(0, sq - L), sq):
                want = v[i, L - sq + j].repeat_interleave(hq // hk, dim=0)
                assert torch.equal(out[i, j].float().cpu(), want)


@pytest.mark.parametrize("ps", [None, 16])
@pytest.mark.parametrize("dtype,d", [(BF16, 128), (FP16, 64)])
def test_fp8_against_dequantised_reference(dtype, d, ps):
    _run_case([65, 300, 512], 17, (8, 2), d, dtype, qlens=[17, 5, 17],
              ps=ps, fp8=True, seed=2)
    _run_case([200, 512], 200, (28, 4), d, dtype, ps=ps, fp8=True, seed=3)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("ps", [16, 64])
def test_paged_bitwise_equals_gathered(ps, fp8):
    """Permuted pages, a physical page shared by all sequences and a strided
    pool: bitwise the contiguous kernel on the gathered cache."""
    from torchacc_amd.ops.flash_attn import _gather_pages
    fn = _fn()
    b, sq, hq, hk, d = 3, 64, 8, 2, 128
    q, k, v = _make(b, sq, hq, hk, d, BF16, seed=5)
    k[1:, :ps] = k[0, :ps]           # the shared prefix page
    v[1:, :ps] = v[0, :ps]
    kw = {}
    if fp8:
        ks, vs = _scales(hk, 5)
        gk, gv = _quant(k, ks).cuda(), _quant(v, vs).cuda()
        kw = {"k_scale": ks.cuda(), "v_scale": vs.cuda()}
    else:
        gk, gv = _gpu(k, BF16), _gpu(v, BF16)
    gq = _gpu(q, BF16)
    lens, qlens = _i32([300, 512, 70]).cuda(), _i32([64, 9, 33]).cuda()
    for wl in (-1, 100):
        want = fn(gq, gk, gv, lens, q_seqlens=qlens, window_size=(wl, -1),
                  return_lse=True, **kw)
        for strided in (False, True):
            kp, vp, table, _ = _paginate(gk, gv, ps, seed=ps, share=True,
                                         strided=strided)
            assert kp.is_contiguous() != strided
            assert int(table[1, 0]) == int(table[0, 0])
            gathered = fn(gq, _gather_pages(kp, table),
                          _gather_pages(vp, table), lens, q_seqlens=qlens,
                          window_size=(wl, -1), return_lse=True, **kw)
            got = fn(gq, kp, vp, lens, q_seqlens=qlens, window_size=(wl, -1),
                     return_lse=True, block_table=table, **kw)
            for a, g_, w_ in zip(got, gathered, want):
                assert torch.equal(a, g_) and torch.equal(a, w_)
            got64 = fn(gq, kp, vp, lens, q_seqlens=qlens,
                       window_size=(wl, -1), return_lse=True,
                       block_table=table.long(), **kw)
            assert torch.equal(got64[0], got[0])


def test_ragged_batch_rows_and_decode_agreement():
    """n = 1 is a decode step: that row agrees with flash_attn_with_kvcache
    for its sequence; rows at or past n (and rows with p < 0) are exactly zero
    with lse = -inf."""
    fn, decode = _ops()
    lens, qlens, sq = [300, 512, 0, 40, 5], [1, 17, 4, 0, 9], 17
    out, lse = _run_case(lens, sq, (8, 2), 128, BF16, qlens=qlens, seed=6)
    q, k, v = _make(5, sq, 8, 2, 128, BF16, seed=6)
    gq, gk, gv = (_gpu(t, BF16) for t in (q, k, v))
    want, want_lse = decode(gq[0:1, 0:1], gk[0:1], gv[0:1],
                            cache_seqlens=_i32([300]).cuda(),
                            return_lse=True)
    err = float((out[0, 0].float() - want[0, 0].float()).abs().max())
    assert err <= OUT_REL * float(want.float().abs().max()), err
    assert float((lse[0, :, 0] - want_lse[0, :, 0]).abs().max()) <= LSE_ABS
    for i, (L, n) in enumerate(zip(lens, qlens)):
        dead = list(range(0, max(0, min(n, sq) - L))) + list(range(n, sq))
        assert bool((out[i, dead] == 0).all())
        assert bool((lse[i][:, dead] == float("-inf")).all())


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("wl,ps", [(-1, None), (100, None), (-1, 16),
                                   (16, 64)])
def test_poisoned_slots_pages_and_table_entries_cannot_matter(wl, ps, fp8):
    """NaN in every slot at or past L, below the window of the first row and
    in unreferenced pages; table entries past the live pages out of range:
    bitwise the result on clean inputs."""
    args = ([65, 300, 0, 130], 64, (8, 2), 128, BF16)
    kw = dict(qlens=[64, 17, 5, 64], wl=wl, ps=ps, fp8=fp8, seed=7)
    clean = _run_case(*args, **kw)
    dirty = _run_case(*args, poison=True, **kw)
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1])


def test_determinism():
    fn = _fn()
    q, k, v = _make(3, 200, 28, 4, 128, BF16, seed=8)
    gq, gk, gv = (_gpu(t, BF16) for t in (q, k, v))
    lens = _i32([257, 512, 199]).cuda()
    a = fn(gq, gk, gv, lens, return_lse=True)
    b = fn(gq, gk, gv, lens, return_lse=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_graph_capture_follows_lengths_table_and_scales():
    """One captured paged fp8 call; cache_seqlens, q_seqlens, the block table
    and both scales are device buffers read at replay."""
    from torchacc_amd.ops.flash_attn import (_gather_pages, _ref_chunk,
                                             dequantize_kv_fp8)
    fn = _fn()
    b, sq, hq, hk, d, ps = 2, 17, 8, 2, 128, 16
    q, k, v = _make(b, sq, hq, hk, d, BF16, seed=9)
    ks, vs = _scales(hk, 9)
    k8, v8 = _quant(k, ks), _quant(v, vs)
    kp, vp, table, _ = _paginate(k8.cuda(), v8.cuda(), ps, seed=1)
    gq = _gpu(q, BF16)
    lens, qlens = _i32([40, 70]).cuda(), _i32([17, 17]).cuda()
    gks, gvs = ks.cuda(), vs.cuda()

    def call():
        return fn(gq, kp, vp, lens, q_seqlens=qlens, return_lse=True,
                  block_table=table, k_scale=gks, v_scale=gvs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = call()

    def replay_and_check(tag):
        graph.replay()
        eager, eager_lse = call()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(lse, eager_lse)
        kc = dequantize_kv_fp8(_gather_pages(kp, table).cpu(), gks.cpu())
        vc = dequantize_kv_fp8(_gather_pages(vp, table).cpu(), gvs.cpu())
        ref, ref_lse = _ref_chunk(q, kc, vc, lens.cpu(), qlens.cpu(),
                                  1.0 / math.sqrt(d), -1)
        _check(out, lse, ref, ref_lse, BF16, d, tag)

    replay_and_check("graph lens [40, 70]")
    lens.copy_(_i32([300, 512]))
    replay_and_check("graph lens [300, 512]")
    qlens.copy_(_i32([1, 9]))
    replay_and_check("graph q_seqlens [1, 9]")
    # another page assignment of the same data, written in place
    kp2, vp2, table2, _ = _paginate(k8.cuda(), v8.cuda(), ps, seed=2)
    assert not torch.equal(table2, table)
    kp.copy_(kp2)
    vp.copy_(vp2)
    table.copy_(table2)
    replay_and_check("graph new table")
    gks.mul_(1.5)
    gvs.mul_(0.5)
    replay_and_check("graph new scales")


@pytest.mark.parametrize("dtype,d,ps", [(torch.float32, 64, None),
                                        (BF16, 96, None), (BF16, 64, 8),
                                        (torch.float32, 128, 16)])
def test_uncovered_inputs_stay_on_the_gpu(dtype, d, ps):
    """fp32, head dim 96 and page size 8 run the fp32 composite on the device
    (same arithmetic as the CPU reference: one output ulp / fp32 summation
    order apart at most)."""
    from torchacc_amd.ops.flash_attn import _ref_chunk
    fn = _fn()
    cap = 64
    q, k, v = _make(3, 5, 4, 2, d, dtype, seed=10, cap=cap)
    lens, qlens = _i32([5, 0, 33]), _i32([5, 2, 3])
    ref, ref_lse = _ref_chunk(q, k, v, lens, qlens, 1.0 / math.sqrt(d), 8)
    gk, gv = _gpu(k, dtype), _gpu(v, dtype)
    kw = {}
    if ps is not None:
        gk, gv, table, _ = _paginate(gk, gv, ps)
        kw["block_table"] = table
    out, lse = fn(_gpu(q, dtype), gk, gv, lens.cuda(),
                  q_seqlens=qlens.cuda(), window_size=(8, -1),
                  return_lse=True, **kw)
    assert out.is_cuda and out.dtype == dtype and lse.is_cuda
    oerr, lerr = _errs(out, lse, ref, ref_lse)
    print(f"uncovered {dtype} d{d} ps{ps}: out {oerr:.3e} lse {lerr:.3e}")
    assert oerr <= (1e-4 if dtype == torch.float32 else 2.0 ** -7)
    assert lerr <= 1e-4


def test_argument_errors_on_the_gpu():
    fn = _fn()
    q, k, v = _make(2, 3, 8, 2, 64, BF16, cap=128)
    gq, gk, gv = (_gpu(t, BF16) for t in (q, k, v))
    lens = _i32([5, 100]).cuda()
    a = fn(gq, gk, gv, lens)
    b = fn(gq, gk, gv, torch.tensor([5, 100]).cuda())      # int64 lengths
    assert torch.equal(a, b)
    with pytest.raises(AssertionError):       # lens on the wrong device
        fn(gq, gk, gv, _i32([5, 100]))
    with pytest.raises(RuntimeError):
        fn(gq.clone().requires_grad_(), gk, gv, lens)
    wide = torch.zeros(2, 128, 2, 128, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError):         # [heads][d] not dense
        fn(gq, wide[..., :64], wide[..., :64], lens)


def test_chunked_prefill_end_to_end(monkeypatch):
    """Tiny Llama, bf16, paged cache (page 16), 48-token prompt in chunks of
    16: the last-position logits are as close to an fp32 CPU run of the same
    weights as the unchunked GPU prefill is (within a factor 2), and no
    gathered copy of the cache is made."""
    import copy
    from torchacc_amd.models import LlamaConfig, LlamaForCausalLM
    from torchacc_amd.models import generation as G
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=1024, hidden_size=512,
                      intermediate_size=1024, num_hidden_layers=2,
                      num_attention_heads=8, num_key_value_heads=2,
                      max_position_embeddings=128)
    with torch.device("cuda"):
        model = LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    assert model.layers[0].self_attn.head_dim == 64
    ref_model = copy.deepcopy(model).float().cpu().eval()
    ids = torch.randint(0, 1024, (2, 48), device="cuda")
    with torch.no_grad():
        want = ref_model(ids.cpu())[:, -1].float()

    def no_gather(*a, **kw):
        raise AssertionError("PagedKVCache.gather must not be called")

    monkeypatch.setattr(G.PagedKVCache, "gather", no_gather)
    calls = []
    real = G.flash_attn_chunk_with_kvcache

    def counted(*a, **kw):
        calls.append(a[0].shape[1])
        return real(*a, **kw)

    monkeypatch.setattr(G, "flash_attn_chunk_with_kvcache", counted)

    def prefill(chunk):
        pool = G.PagedKVCache.for_model(model, 2, 2 * 3, 16, 48)
        with torch.no_grad():
            return G._prefill(model, ids, pool, chunk).float().cpu()

    err_whole = float((prefill(None) - want).abs().max())
    assert calls == []
    err_chunk = float((prefill(16) - want).abs().max())
    assert calls == [16] * 4, calls           # 2 later chunks x 2 layers
    print(f"last-position logits vs fp32 CPU: unchunked {err_whole:.3e} "
          f"chunked {err_chunk:.3e}")
    assert err_chunk <= 2.0 * err_whole, (err_chunk, err_whole)
    out = model.generate(ids, max_new_tokens=4, page_size=16,
                         prefill_chunk=16)
    assert out.shape == (2, 52)
