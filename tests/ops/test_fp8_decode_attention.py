"""GPU numerics of the fp8 (e4m3fn) KV cache: the fp8 variant of the split-KV
decode kernel (contiguous and paged), the quantising cache write, and
generation on top of them.

Every decode case is compared with the fp32 CPU reference on the dequantised
cache (codes.float() * scale), so quantisation error is not part of the
bounds, which are those of test_decode_attention.py:
        out  max|got - ref| <= 1.5e-2 * max|ref|
        lse  max|got - ref| <= 1e-2
The kernel's arithmetic is the 16-bit kernel's plus one fp32 multiply per q
element and per output element. Scales are per head and no powers of two
unless a test needs exactness.

Exact checks: paged fp8 is bitwise contiguous fp8 on the gathered cache at the
same num_splits (same key-to-lane mapping, tile loop, split chunks, merge
order); a call repeated gives the same bits; poisoned slots and pages (byte
0x7f, the NaN code) cannot change a bit.

No test uses an out-of-range slot or page index.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

OUT_REL = 1.5e-2
LSE_ABS = 1e-2
BF16, FP16 = torch.bfloat16, torch.float16
FP8 = torch.float8_e4m3fn
CAP = 1024
NAN_CODE = 0x7f


def _op():
    from torchacc_amd.ops import flash_attn_with_kvcache
    return flash_attn_with_kvcache


def _write():
    from torchacc_amd.ops import kv_cache_write_fp8
    return kv_cache_write_fp8


def _u8(t):
    return t.view(torch.uint8)


def _scales(hk, pow2_v=False):
    h = torch.arange(hk, dtype=torch.float32)
    ks = 0.0173 * (1.0 + 0.31 * h)
    vs = torch.full((hk,), 2.0 ** -6) if pow2_v else 0.0119 * (1.0 + 0.23 * h)
    return ks, vs


def _quant(x, scale):
    return (x * (1.0 / scale).view(1, 1, -1, 1)).clamp(-448, 448).to(FP8)


@functools.lru_cache(maxsize=None)
def _make(b, cap, hq, hk, d, dtype, seed=0, pow2_v=False):
    """CPU inputs, shared between tests and never modified in place: q
    rounded to `dtype` (held in fp32), K / V as e4m3 codes, the scales."""
    g = torch.Generator().manual_seed(seed)
    ks, vs = _scales(hk, pow2_v)
    q = torch.randn(b, 1, hq, d, generator=g).to(dtype).float()
    k8 = _quant(torch.randn(b, cap, hk, d, generator=g), ks)
    v8 = _quant(torch.randn(b, cap, hk, d, generator=g), vs)
    return q, k8, v8, ks, vs


@functools.lru_cache(maxsize=None)
def _reference(klens, b, cap, hq, hk, d, dtype, wl, seed=0, pow2_v=False):
    q, k8, v8, ks, vs = _make(b, cap, hq, hk, d, dtype, seed, pow2_v)
    return _op()(q, k8, v8, cache_seqlens=_lens(klens), window_size=(wl, -1),
                 return_lse=True, k_scale=ks, v_scale=vs)


def _lens(vals):
    return torch.tensor(vals, dtype=torch.int32)


def _paginate(k, v, ps, extra=1, seed=1):
    """Cut contiguous fp8 [b, cap, hk, d] caches (any device) into pages at
    permuted physical indices. Returns the pools, the int32 table and the
    indices of `extra` spare pages that no table entry names (zero bytes)."""
    b, cap, hk, d = k.shape
    w = cap // ps
    assert w * ps == cap
    n = b * w + extra
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    table = perm[:b * w].view(b, w).to(torch.int32)
    idx = table.reshape(-1).long().to(k.device)
    pools = []
    for t in (k, v):
        p = torch.zeros(n, ps, hk, d, dtype=torch.uint8, device=t.device)
        p[idx] = _u8(t).reshape(b * w, ps, hk, d)
        pools.append(p.view(FP8))
    return pools[0], pools[1], table.to(k.device), perm[b * w:].tolist()


def _check(out, lse, ref, ref_lse, tag=""):
    out = out.float().cpu()
    lse = lse.float().cpu()
    assert out.shape == ref.shape and lse.shape == ref_lse.shape
    assert bool(torch.isfinite(out).all()), "non-finite output"
    err = float((out - ref).abs().max())
    bound = OUT_REL * float(ref.abs().max())
    empty = torch.isinf(ref_lse)
    got_empty = torch.isinf(lse) & (lse < 0)
    lerr = 0.0
    if bool((~empty).any()):
        lerr = float((lse - ref_lse)[~empty].abs().max())
    print(f"{tag} out err {err:.3e} (bound {bound:.3e})  lse err {lerr:.3e}")
    assert torch.equal(got_empty, empty), "lse = -inf rows differ"
    assert err <= bound, (err, bound)
    assert lerr <= LSE_ABS, lerr


def _same(a, b, tag):
    assert torch.equal(a[0], b[0]), f"{tag}: out differs bitwise"
    assert torch.equal(a[1], b[1]), f"{tag}: lse differs bitwise"


def _run_case(klens, heads, d, dtype, ns, ps, wl=-1, cap=CAP, pow2_v=False):
    """Paged fp8 on a permuted pool vs contiguous fp8 on the cache the pool
    was cut from (bitwise), both vs the fp32 reference (tolerance)."""
    hq, hk = heads
    b = len(klens)
    fn = _op()
    q, k8, v8, ks, vs = _make(b, cap, hq, hk, d, dtype, 0, pow2_v)
    gq = q.to("cuda", dtype)
    gk, gv, gks, gvs = (t.cuda() for t in (k8, v8, ks, vs))
    lens = _lens(klens).cuda()
    kp, vp, table, _ = _paginate(gk, gv, ps)
    kw = dict(cache_seqlens=lens, window_size=(wl, -1), num_splits=ns,
              return_lse=True, k_scale=gks, v_scale=gvs)
    want = fn(gq, gk, gv, **kw)
    got = fn(gq, kp, vp, block_table=table, **kw)
    assert got[0].dtype == dtype and got[1].dtype == torch.float32
    tag = f"{klens} {heads} d{d} ns{ns} ps{ps} wl{wl}"
    _same(got, want, tag)
    _check(*got, *_reference(tuple(klens), b, cap, hq, hk, d, dtype, wl, 0,
                             pow2_v), tag)
    return got


KLENS = [[1, 1], [15, 16], [17, 32], [63, 64], [65, 128], [257, 1000],
         [1024, 0]]

GRID = [(kl, (8, 2), d, BF16, ns, 16)
        for d in (128, 64) for kl in KLENS for ns in (1, 5)] + [
    ([257, 1000], (8, 2), 128, BF16, 0, 16),
    ([257, 1000], (8, 2), 64, BF16, 0, 16),
    ([257, 1000], (4, 4), 64, BF16, 5, 16),
    ([257, 1000], (28, 4), 128, BF16, 5, 16),
    ([65, 128], (32, 2), 64, BF16, 5, 16),
    ([257, 1000], (32, 2), 128, BF16, 0, 16),
    ([257, 1000], (8, 1), 128, BF16, 5, 16),
    ([257, 1000], (28, 4), 128, FP16, 0, 16),
    ([63, 64], (4, 4), 64, FP16, 1, 16),
    ([257, 1000], (8, 2), 128, BF16, 5, 64),
    ([65, 128], (8, 2), 64, BF16, 1, 64),
    ([257, 1000], (8, 2), 128, BF16, 5, 256),
    ([257, 1000], (4, 4), 64, FP16, 0, 256),
]


@pytest.mark.parametrize("klens,heads,d,dtype,ns,ps", GRID)
def test_reference_bounds_and_paged_bitwise(klens, heads, d, dtype, ns, ps):
    _run_case(klens, heads, d, dtype, ns, ps)


@pytest.mark.parametrize("ns", [1, 5])
@pytest.mark.parametrize("wl", [0, 16, 100])
def test_window(wl, ns):
    """lo = 64, 48, 0 and 299, 283, 199: not page- or tile-aligned. With one
    visible key p = 1 and, v_scale being a power of two, the output is that
    key's dequantised V row exactly."""
    klens = [65, 300]
    out, _ = _run_case(klens, (8, 2), 128, BF16, ns, 16, wl=wl, pow2_v=True)
    if wl == 0:
        _, _, v8, _, vs = _make(2, CAP, 8, 2, 128, BF16, 0, True)
        for i, n in enumerate(klens):
            want = (v8[i, n - 1].float() * vs.view(-1, 1)).to(BF16)
            want = want.repeat_interleave(4, dim=0)          # [hq, d]
            assert torch.equal(out[i, 0].cpu(), want)


def test_shared_prefix_pages():
    fn = _op()
    q, k8, v8, ks, vs = _make(2, 256, 8, 2, 128, BF16, seed=2)
    k8, v8 = k8.clone(), v8.clone()
    _u8(k8)[1, :48], _u8(v8)[1, :48] = _u8(k8)[0, :48], _u8(v8)[0, :48]
    gq = q.to("cuda", BF16)
    gk, gv, gks, gvs = (t.cuda() for t in (k8, v8, ks, vs))
    lens = _lens([50, 200]).cuda()
    kp, vp, table, _ = _paginate(gk, gv, 16)
    table[1, :3] = table[0, :3]
    ref = fn(q, k8, v8, cache_seqlens=lens.cpu(), return_lse=True,
             k_scale=ks, v_scale=vs)
    for ns in (1, 5):
        kw = dict(cache_seqlens=lens, num_splits=ns, return_lse=True,
                  k_scale=gks, v_scale=gvs)
        want = fn(gq, gk, gv, **kw)
        got = fn(gq, kp, vp, block_table=table, **kw)
        _same(got, want, f"shared prefix ns{ns}")
        _check(*got, *ref, f"shared prefix ns{ns}")


@pytest.mark.parametrize("ns", [1, 5])
@pytest.mark.parametrize("wl", [-1, 100])
def test_poisoned_slots_and_pages_cannot_matter(ns, wl):
    """Every slot outside [lo, len), every unreferenced page and the page
    every unused table entry names hold the byte 0x7f (NaN) in both layouts;
    out and lse are bitwise those of the clean run."""
    fn = _op()
    klens, ps = [257, 1000], 16
    q, k8, v8, ks, vs = _make(2, CAP, 8, 2, 128, BF16)
    gq = q.to("cuda", BF16)
    gks, gvs = ks.cuda(), vs.cuda()
    lens = _lens(klens).cuda()
    clean = _run_case(klens, (8, 2), 128, BF16, ns, ps, wl=wl)
    k8, v8 = k8.clone(), v8.clone()
    for i, n in enumerate(klens):
        lo = max(0, n - 1 - wl) if wl >= 0 else 0
        for t in (k8, v8):
            _u8(t)[i, n:] = NAN_CODE
            _u8(t)[i, :lo] = NAN_CODE
    gk, gv = k8.cuda(), v8.cuda()
    kp, vp, table, spare = _paginate(gk, gv, ps, extra=3)
    for t in (kp, vp):
        _u8(t)[spare] = NAN_CODE
    for i, n in enumerate(klens):
        table[i, (n + ps - 1) // ps:] = spare[i]
    kw = dict(cache_seqlens=lens, window_size=(wl, -1), num_splits=ns,
              return_lse=True, k_scale=gks, v_scale=gvs)
    cont = fn(gq, gk, gv, **kw)
    paged = fn(gq, kp, vp, block_table=table, **kw)
    assert bool(torch.isfinite(cont[0]).all())
    _same(cont, clean, f"poison contiguous ns{ns} wl{wl}")
    _same(paged, clean, f"poison paged ns{ns} wl{wl}")


def test_strided_pool():
    """Pools that are strided views: K with a larger page stride, V with a
    larger slot stride as well (multiples of 8 bytes)."""
    fn = _op()
    hk, d, ps = 2, 128, 16
    q, k8, v8, ks, vs = _make(2, 256, 8, hk, d, BF16, seed=3)
    gq = q.to("cuda", BF16)
    gk, gv, gks, gvs = (t.cuda() for t in (k8, v8, ks, vs))
    kp, vp, table, _ = _paginate(gk, gv, ps)
    n = kp.shape[0]
    row = hk * d
    kbuf = torch.full((n, ps * row + 8 * row), NAN_CODE, dtype=torch.uint8,
                      device="cuda")
    kst = kbuf.as_strided((n, ps, hk, d), (kbuf.stride(0), row, d, 1))
    vbuf = torch.full((n, ps * (row + 8) + 64), NAN_CODE, dtype=torch.uint8,
                      device="cuda")
    vst = vbuf.as_strided((n, ps, hk, d), (vbuf.stride(0), row + 8, d, 1))
    kst.copy_(_u8(kp))
    vst.copy_(_u8(vp))
    kst, vst = kst.view(FP8), vst.view(FP8)
    assert not kst.is_contiguous() and not vst.is_contiguous()
    lens = _lens([77, 256]).cuda()
    ref = fn(q, k8, v8, cache_seqlens=lens.cpu(), return_lse=True,
             k_scale=ks, v_scale=vs)
    for ns in (1, 3):
        kw = dict(cache_seqlens=lens, num_splits=ns, return_lse=True,
                  k_scale=gks, v_scale=gvs)
        want = fn(gq, gk, gv, **kw)
        got = fn(gq, kst, vst, block_table=table, **kw)
        _same(got, want, f"strided pool ns{ns}")
        _check(*got, *ref, f"strided pool ns{ns}")


def test_page_stride_past_2_31_elements():
    """The second page lies more than 2^31 elements (= bytes) from the
    first: page offsets must be computed in 64 bits."""
    fn = _op()
    hk, d, ps = 2, 128, 64
    q, k8, v8, ks, vs = _make(2, 2 * ps, 8, hk, d, BF16, seed=4)
    stride_p = 2 ** 31 + 8 * hk * d
    n = ps * hk * d
    buf = torch.empty(stride_p + 2 * n, dtype=torch.uint8, device="cuda")
    kp = buf.as_strided((2, ps, hk, d), (stride_p, hk * d, d, 1), 0)
    vp = buf.as_strided((2, ps, hk, d), (stride_p, hk * d, d, 1), n)
    table = torch.tensor([[1, 0], [1, 0]], dtype=torch.int32, device="cuda")
    for pool, src in ((kp, k8), (vp, v8)):
        pool[1].copy_(_u8(src)[0, :ps])
        pool[0].copy_(_u8(src)[0, ps:])
    kc = torch.stack([_u8(k8)[0], _u8(k8)[0]]).view(FP8)
    vc = torch.stack([_u8(v8)[0], _u8(v8)[0]]).view(FP8)
    lens = _lens([2 * ps - 5, 40])
    ref = fn(q, kc, vc, cache_seqlens=lens, return_lse=True, k_scale=ks,
             v_scale=vs)
    gq = q.to("cuda", BF16)
    kw = dict(cache_seqlens=lens.cuda(), return_lse=True, k_scale=ks.cuda(),
              v_scale=vs.cuda())
    want = fn(gq, kc.cuda(), vc.cuda(), **kw)
    got = fn(gq, kp.view(FP8), vp.view(FP8), block_table=table, **kw)
    _same(got, want, "2^31 page stride")
    _check(*got, *ref, "2^31 page stride")


def test_determinism():
    fn = _op()
    q, k8, v8, ks, vs = _make(2, CAP, 8, 2, 128, BF16)
    gq = q.to("cuda", BF16)
    gk, gv, gks, gvs = (t.cuda() for t in (k8, v8, ks, vs))
    kp, vp, table, _ = _paginate(gk, gv, 16)
    lens = _lens([257, 1000]).cuda()
    for ns in (1, 5, 0):
        kw = dict(cache_seqlens=lens, num_splits=ns, return_lse=True,
                  k_scale=gks, v_scale=gvs)
        _same(fn(gq, gk, gv, **kw), fn(gq, gk, gv, **kw),
              f"determinism contiguous ns{ns}")
        _same(fn(gq, kp, vp, block_table=table, **kw),
              fn(gq, kp, vp, block_table=table, **kw),
              f"determinism paged ns{ns}")


def test_graph_capture_follows_lengths_table_and_scales():
    fn, write = _op(), _write()
    q, k8, v8, ks, vs = _make(2, CAP, 8, 2, 128, BF16)
    gq = q.to("cuda", BF16)
    gk, gv, gks, gvs = (t.cuda() for t in (k8, v8, ks, vs))
    kp, vp, table, _ = _paginate(gk, gv, 16)
    lens = _lens([40, 70]).cuda()
    kw = dict(cache_seqlens=lens, num_splits=5, return_lse=True,
              block_table=table, k_scale=gks, v_scale=gvs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(gq, kp, vp, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = fn(gq, kp, vp, **kw)

    def replay_and_check(tag):
        graph.replay()
        eager = fn(gq, kp, vp, **kw)
        torch.cuda.synchronize()
        _same((out, lse), eager, tag)
        ref = fn(q, gk.cpu(), gv.cpu(), cache_seqlens=lens.cpu(),
                 return_lse=True, k_scale=gks.cpu(), v_scale=gvs.cpu())
        _check(out, lse, *ref, tag)

    replay_and_check("graph [40, 70]")
    # append one token per sequence through the write op, as a decode step
    # does: into the contiguous twin and into the pool
    g = torch.Generator().manual_seed(7)
    new_k = torch.randn(2, 1, 2, 128, generator=g).to("cuda", BF16)
    new_v = torch.randn(2, 1, 2, 128, generator=g).to("cuda", BF16)
    pos = torch.tensor([40, 70], device="cuda")
    write(new_k, new_v, gk, gv, torch.arange(2, device="cuda") * CAP + pos,
          gks, gvs)
    page = table.gather(1, (pos // 16).view(2, 1)).view(2).long()
    write(new_k, new_v, kp, vp, page * 16 + pos % 16, gks, gvs)
    lens.add_(1)
    replay_and_check("graph [41, 71]")
    # longer lengths and another page assignment: only device buffers change
    kp2, vp2, table2, _ = _paginate(gk, gv, 16, seed=9)
    assert not torch.equal(table2, table)
    kp.copy_(kp2)
    vp.copy_(vp2)
    table.copy_(table2)
    lens.copy_(_lens([200, 300]))
    replay_and_check("graph [200, 300], new table")
    # other values in the scale buffers: read at replay
    gks.mul_(1.7)
    gvs.mul_(0.6)
    replay_and_check("graph, new scales")


def _order(codes_u8):
    """e4m3 bytes -> integers ordered like the values (+0 and -0 both 0)."""
    c = codes_u8.to(torch.int32)
    mag = c & 0x7f
    return torch.where(c >= 128, -mag, mag)


def _special(hk, d, dtype):
    vals = [1000.0, -1000.0, 448.0, -448.0, 449.0, 464.0, 17.0, 18.0, 19.0,
            -17.0, -19.0, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -10,
            2.0 ** -11, -2.0 ** -12, 1e-8, 0.0, 0.3, -5.7]
    row = torch.tensor(vals).repeat((hk * d + len(vals) - 1) // len(vals))
    return row[:hk * d].view(hk, d).to(dtype)


@pytest.mark.parametrize("dtype,idx,d", [(BF16, torch.int64, 128),
                                         (FP16, torch.int32, 64),
                                         (BF16, torch.int32, 40)])
def test_write_op(dtype, idx, d):
    """GPU codes against the CPU op's: bitwise for power-of-two scales
    (ties, saturation, subnormals included), equal or adjacent for arbitrary
    scales; permuted slots, a strided pool, untouched slots stay poisoned."""
    write = _write()
    b, s, hk, n0, n1 = 2, 3, 2, 5, 16
    g = torch.Generator().manual_seed(11)
    k = (torch.randn(b, s, hk, d, generator=g) * 30).to(dtype)
    v = (torch.randn(b, s, hk, d, generator=g) * 2).to(dtype)
    k[0, 0] = _special(hk, d, dtype)
    v[1, 2] = _special(hk, d, dtype)
    slots = torch.tensor([9, 79, 0, 17, 33, 62], dtype=idx)
    for pow2 in (True, False):
        if pow2:
            ks, vs = torch.tensor([0.5, 4.0]), torch.tensor([2.0, 0.125])
        else:
            ks, vs = torch.tensor([0.37, 1.9]), torch.tensor([0.011, 0.73])
        cpu = [torch.full((n0, n1, hk, d), 0x5a, dtype=torch.uint8).view(FP8)
               for _ in range(2)]
        write(k, v, cpu[0], cpu[1], slots, ks, vs)
        # a strided pool: slot stride hk * d + 8 bytes, padded pages
        bufs = [torch.full((n0, n1 * (hk * d + 8) + 24), 0x5a,
                           dtype=torch.uint8, device="cuda")
                for _ in range(2)]
        gpu = [t.as_strided((n0, n1, hk, d),
                            (t.stride(0), hk * d + 8, d, 1)).view(FP8)
               for t in bufs]
        write(k.cuda(), v.cuda(), gpu[0], gpu[1], slots.cuda(), ks.cuda(),
              vs.cuda())
        torch.cuda.synchronize()
        for buf, got, want in zip(bufs, gpu, cpu):
            got, want = _u8(got).cpu(), _u8(want)
            # the padding bytes of the strided buffer are untouched
            exp = torch.full(buf.shape, 0x5a, dtype=torch.uint8)
            exp.as_strided(got.shape, (exp.stride(0), hk * d + 8, d, 1)) \
                .copy_(got)
            assert torch.equal(buf.cpu(), exp)
            if pow2:
                assert torch.equal(got, want)
            else:
                diff = (_order(got) - _order(want)).abs()
                print(f"codes differing by one step: {int((diff > 0).sum())}")
                assert int(diff.max()) <= 1
                assert not bool(((got & 0x7f) == NAN_CODE).any())
            rest = torch.ones(n0 * n1, dtype=torch.bool)
            rest[slots.long()] = False
            assert bool((got.reshape(n0 * n1, hk, d)[rest] == 0x5a).all())


@pytest.mark.parametrize("dtype,d,ps", [(torch.float32, 64, 16),
                                        (BF16, 96, 16), (BF16, 128, 24)])
def test_uncovered_inputs_stay_on_the_gpu(dtype, d, ps):
    """fp32 q, head dims other than 64/128 and page sizes that are no power
    of two >= 16 dequantise a copy on the device and take the existing
    fallback paths, in both layouts."""
    fn = _op()
    q, k8, v8, ks, vs = _make(3, 48, 4, 2, d, dtype, seed=5)
    lens = _lens([5, 0, 33])
    ref = fn(q, k8, v8, cache_seqlens=lens, return_lse=True, k_scale=ks,
             v_scale=vs)
    gk, gv = k8.cuda(), v8.cuda()
    kw = dict(cache_seqlens=lens.cuda(), return_lse=True, k_scale=ks.cuda(),
              v_scale=vs.cuda())
    kp, vp, table, _ = _paginate(gk, gv, ps)
    out, lse = fn(q.to("cuda", dtype), kp, vp, block_table=table, **kw)
    assert out.is_cuda and lse.is_cuda and out.dtype == dtype
    _check(out, lse, *ref, f"paged fallback {dtype} d{d} ps{ps}")
    if ps == 16:
        out, lse = fn(q.to("cuda", dtype), gk, gv, **kw)
        assert out.is_cuda and out.dtype == dtype
        _check(out, lse, *ref, f"contiguous fallback {dtype} d{d}")


def test_generation_end_to_end(monkeypatch):
    """generate(kv_dtype="fp8"), its paged form and both GraphDecoder forms
    return identical tokens (capacities < 512: one split everywhere, same
    key ranges, same codes and scales); every decode step passes fp8 caches;
    the first new token is the bf16 path's, since prefill never reads the
    cache."""
    from torchacc_amd.models import LlamaConfig, LlamaForCausalLM
    from torchacc_amd.models import generation
    calls = []
    real = generation.flash_attn_with_kvcache

    def counted(*a, **kw):
        calls.append((a[1].dtype, a[2].dtype,
                      kw.get("block_table") is not None,
                      kw.get("k_scale") is not None
                      and kw.get("v_scale") is not None))
        return real(*a, **kw)

    monkeypatch.setattr(generation, "flash_attn_with_kvcache", counted)
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=1024, hidden_size=1024,
                      intermediate_size=2048, num_hidden_layers=2,
                      num_attention_heads=8, num_key_value_heads=2,
                      max_position_embeddings=256)
    with torch.device("cuda"):
        model = LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    ids = torch.randint(0, 1024, (2, 60), device="cuda")
    ids2 = torch.randint(0, 1024, (2, 45), device="cuda")
    base = model.generate(ids, max_new_tokens=12)
    calls.clear()
    cont = model.generate(ids, max_new_tokens=12, kv_dtype="fp8")
    # 11 decode steps x 2 layers
    assert calls == [(FP8, FP8, False, True)] * (11 * 2), calls
    assert torch.equal(cont[:, :61], base[:, :61])
    calls.clear()
    paged = model.generate(ids, max_new_tokens=12, kv_dtype="fp8",
                           page_size=16)
    assert calls == [(FP8, FP8, True, True)] * (11 * 2), calls
    assert torch.equal(paged, cont), (paged[:, 60:], cont[:, 60:])

    pool = generation.PagedKVCache.for_model(model, 2, 2 * 5, 16, 72,
                                             kv_dtype="fp8")
    again = model.generate(ids, max_new_tokens=12, kv_pool=pool)
    assert torch.equal(again, cont) and len(pool.free_pages) == 10

    want2 = model.generate(ids2, max_new_tokens=12, kv_dtype="fp8")
    for page_size in (None, 16):
        calls.clear()
        dec = generation.GraphDecoder(model, 2, 128, page_size=page_size,
                                      kv_dtype="fp8")
        got = dec.decode(ids, 12)
        torch.cuda.synchronize()
        # two warm-up steps and the captured one, 2 layers each
        assert calls == [(FP8, FP8, page_size is not None, True)] * 6, calls
        assert torch.equal(got, cont), (got[:, 60:], cont[:, 60:])
        # another prompt, other scales: the captured step reads the scale
        # buffers at replay, no recapture
        calls.clear()
        scale_before = [c.k_scale.clone() for c in dec.caches]
        got2 = dec.decode(ids2, 12)
        torch.cuda.synchronize()
        assert calls == []
        assert any(not torch.equal(c.k_scale, s)
                   for c, s in zip(dec.caches, scale_before))
        assert torch.equal(got2, want2), (got2[:, 45:], want2[:, 45:])
