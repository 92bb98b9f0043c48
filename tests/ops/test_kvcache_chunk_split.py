"""GPU numerics of split-KV in flash_attn_chunk_with_kvcache (``num_splits``,
csrc/flash_attn_kvcache_mq.hip: the SPLIT instances and the combine kernel).

Reference, error measures and bounds are those of test_kvcache_chunk.py,
whose helpers are imported: ``_ref_chunk`` in fp32 on inputs rounded to the
kernel dtype; out: max|got - ref| / max|ref|, lse: max|got - ref| over the rows
that see a key; bound = 1.5 * old + 1e-3 for both, ``old`` being fa_forward's
largest error over the expressible cases of the same dtype and head dim,
computed in the run. The partials are fp32 and the output is rounded once, so
the split result gets no looser bound than the unsplit one.

Every test passes ``num_splits=``. Shapes: cap 512 (8 tiles of 64 keys) unless
stated, b <= 5. With lens [300, 512, 65, 0, 40], q_lens [64, 17, 64, 4, 9],
sq 64 and heads (8, 2) (two 128-row tiles per kv head) the workgroups own
5, 5, 8, 8, 1, 2, 0, 0, 1 and 0 tiles: 5 tiles over 3 splits (2, 2, 1), 2
tiles over 4 and 9 splits, an all-empty sequence, rows with p < 0, rows
j >= n, a row tile without a valid row, and causal rows whose position lies
below a later split's first key (sequence 0, rows at 236..267 against the
split that starts at key 256).
"""
import functools
import math

import pytest
import torch

from tests.ops.test_kvcache_chunk import (BF16, CAP, FP16, _check, _fn, _gpu,
                                          _i32, _make, _paginate, _quant,
                                          _scales, _visible_union)

pytestmark = pytest.mark.gpu

SPLITS = [2, 3, 4, 9]
# (lens, q_lens, sq, heads)
RAGGED = ((300, 512, 65, 0, 40), (64, 17, 64, 4, 9), 64, (8, 2))
SHAPES = [
    RAGGED,
    ((257, 512, 200), None, 200, (28, 4)),     # 11 row tiles, each its range
    ((300, 512, 65, 0, 2), None, 1, (8, 2)),
    ((300, 512, 65, 0, 2), None, 3, (8, 2)),   # L = 2 < n = 3: a row at p < 0
    ((300, 512, 65, 0, 2), None, 1, (32, 2)),
    ((300, 512, 65, 0, 2), None, 3, (32, 2)),
]
LAYOUTS = [(None, False), (16, False), (None, True), (16, True)]  # (page, fp8)


@functools.lru_cache(maxsize=None)
def _case(lens, qlens, sq, heads, d, dtype, wl, fp8, seed, cap=CAP):
    """CPU inputs and the fp32 reference of one case, computed once and shared
    by every num_splits / layout that runs it. Nothing in it is modified."""
    from torchacc_amd.ops.flash_attn import _ref_chunk, dequantize_kv_fp8
    hq, hk = heads
    q, k, v = _make(len(lens), sq, hq, hk, d, dtype, seed=seed, cap=cap)
    c = {"q": q, "k": k, "v": v, "scales": None}
    if fp8:
        ks, vs = _scales(hk, seed)
        c["k8"], c["v8"] = _quant(k, ks), _quant(v, vs)
        c["scales"] = (ks, vs)
        k = dequantize_kv_fp8(c["k8"], ks)
        v = dequantize_kv_fp8(c["v8"], vs)
    ql = None if qlens is None else _i32(list(qlens))
    c["ref"], c["ref_lse"] = _ref_chunk(q, k, v, _i32(list(lens)), ql,
                                        1.0 / math.sqrt(d), wl)
    return c


def _device_inputs(lens, qlens, sq, heads, d, dtype, wl=-1, ps=None,
                   fp8=False, poison=False, seed=0, cap=CAP):
    """(case, positional args, keyword args) of the op for one case."""
    c = _case(tuple(lens), None if qlens is None else tuple(qlens), sq, heads,
              d, dtype, wl, fp8, seed, cap)
    b = len(lens)
    kw = {}
    if fp8:
        gk, gv = c["k8"].cuda(), c["v8"].cuda()
        kw = {"k_scale": c["scales"][0].cuda(), "v_scale": c["scales"][1].cuda()}
    else:
        gk, gv = _gpu(c["k"], dtype), _gpu(c["v"], dtype)
    if poison:
        nan = 0x7f if fp8 else float("nan")       # 0x7f is NaN in e4m3fn
        for i in range(b):
            lo, hi = _visible_union(lens[i], sq if qlens is None
                                    else qlens[i], sq, wl, cap)
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
                live = -(-min(max(lens[i], 0), cap) // ps)
                table[i, live:] = 2 ** 30 if i % 2 else -7
    if qlens is not None:
        kw["q_seqlens"] = _i32(list(qlens)).cuda()
    kw["window_size"] = (wl, -1)
    args = (_gpu(c["q"], dtype), gk, gv, _i32(list(lens)).cuda())
    return c, args, kw


def _call_and_check(c, args, kw, num_splits, dtype, d, tag):
    out, lse = _fn()(*args, return_lse=True, num_splits=num_splits, **kw)
    assert out.dtype == dtype and lse.dtype == torch.float32
    _check(out, lse, c["ref"], c["ref_lse"], dtype, d,
           f"{tag} num_splits={num_splits}")
    # rows that see nothing: exactly zero (lse = -inf is asserted by _check)
    dead = torch.isinf(c["ref_lse"]).permute(0, 2, 1)         # [b, sq, hq]
    assert bool((out.cpu()[dead] == 0).all()), tag
    return out, lse


# ---- 1. parity grid ---------------------------------------------------------
@pytest.mark.parametrize("ps,fp8", LAYOUTS)
@pytest.mark.parametrize("d,dtype", [(64, BF16), (128, BF16), (64, FP16),
                                     (128, FP16)])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_parity_grid(shape, d, dtype, ps, fp8):
    lens, qlens, sq, heads = SHAPES[shape]
    c, args, kw = _device_inputs(lens, qlens, sq, heads, d, dtype, ps=ps,
                                 fp8=fp8, seed=shape)
    for ns in SPLITS:
        _call_and_check(c, args, kw, ns, dtype, d,
                        f"L{lens} n{qlens} sq{sq} {heads} d{d} {dtype} "
                        f"ps{ps} fp8={fp8}")


# ---- 2. windows: t0 moves, the cut starts mid-cache --------------------------
@pytest.mark.parametrize("wl", [0, 16, 100])
@pytest.mark.parametrize("sq,heads,ps", [(17, (8, 2), None),
                                         (200, (28, 4), 16)])
def test_window(wl, sq, heads, ps):
    lens = (65, 300, 512)
    c, args, kw = _device_inputs(lens, None, sq, heads, 128, BF16, wl=wl,
                                 ps=ps, seed=11)
    _call_and_check(c, args, kw, 3, BF16, 128,
                    f"window {wl} sq{sq} {heads} ps{ps}")


# ---- 3. num_splits=1 is the default at cap 512 -------------------------------
@pytest.mark.parametrize("ps,fp8", LAYOUTS)
def test_one_split_is_the_default(ps, fp8):
    lens, qlens, sq, heads = RAGGED
    _, args, kw = _device_inputs(lens, qlens, sq, heads, 128, BF16, ps=ps,
                                 fp8=fp8)
    fn = _fn()
    one = fn(*args, return_lse=True, num_splits=1, **kw)
    default = fn(*args, return_lse=True, **kw)
    auto = fn(*args, return_lse=True, num_splits=0, **kw)
    for a, b_, c_ in zip(one, default, auto):
        assert torch.equal(a, b_) and torch.equal(a, c_)


# ---- 4. paged equals gathered, bitwise ----------------------------------------
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("ps", [16, 64])
def test_paged_bitwise_equals_gathered(ps, fp8):
    """Permuted pages, a physical page shared by all sequences and a strided
    pool: bitwise the contiguous kernel on the gathered cache at the same
    num_splits."""
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
        kw.update(q_seqlens=qlens, window_size=(wl, -1), return_lse=True,
                  num_splits=3)
        want = fn(gq, gk, gv, lens, **kw)
        for strided in (False, True):
            kp, vp, table, _ = _paginate(gk, gv, ps, seed=ps, share=True,
                                         strided=strided)
            assert kp.is_contiguous() != strided
            assert int(table[1, 0]) == int(table[0, 0])
            gathered = fn(gq, _gather_pages(kp, table),
                          _gather_pages(vp, table), lens, **kw)
            got = fn(gq, kp, vp, lens, block_table=table, **kw)
            for a, g_, w_ in zip(got, gathered, want):
                assert torch.equal(a, g_) and torch.equal(a, w_)


# ---- 5. poison -----------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("wl,ps", [(-1, None), (100, None), (-1, 16),
                                   (16, 64)])
def test_poisoned_slots_pages_table_entries_and_workspace(wl, ps, fp8):
    """NaN in every slot at or past L, below the window of the first row and
    in unreferenced pages; table entries past the live pages out of range;
    and a workspace that most likely holds NaN (an fp32 block of its size is
    NaN-filled and freed right before the call, so the caching allocator can
    hand it to torch.empty): finite, and bitwise the clean result. An empty
    split's partial row that the combine read by mistake would show here."""
    lens, qlens, sq, heads, d, ns = [65, 300, 0, 130], [64, 17, 5, 64], 64, \
        (8, 2), 128, 4
    spec = dict(wl=wl, ps=ps, fp8=fp8, seed=7)
    c, args, kw = _device_inputs(lens, qlens, sq, heads, d, BF16, **spec)
    clean = _call_and_check(c, args, kw, ns, BF16, d, f"clean wl{wl} ps{ps}")
    c, args, kw = _device_inputs(lens, qlens, sq, heads, d, BF16, poison=True,
                                 **spec)
    rows = len(lens) * sq * heads[0]
    torch.cuda.synchronize()
    junk = [torch.full((rows * ns * d,), float("nan"), device="cuda"),
            torch.full((rows * ns,), float("nan"), device="cuda")]
    del junk
    dirty = _call_and_check(c, args, kw, ns, BF16, d, f"dirty wl{wl} ps{ps}")
    assert bool(torch.isfinite(dirty[0].float()).all())
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1])


# ---- 6. determinism ------------------------------------------------------------
def test_determinism():
    _, args, kw = _device_inputs((257, 512, 199), None, 200, (28, 4), 128,
                                 BF16, seed=8)
    fn = _fn()
    a = fn(*args, return_lse=True, num_splits=3, **kw)
    b = fn(*args, return_lse=True, num_splits=3, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 7. graph capture ----------------------------------------------------------
def test_graph_capture_follows_lengths_table_and_scales():
    """One captured paged fp8 call at num_splits 4 (two launches and the
    workspace inside the graph); lengths, table and scales are device buffers
    read at replay. At lens [40, 70] three of the four splits are empty."""
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
                  block_table=table, k_scale=gks, v_scale=gvs, num_splits=4)

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
    kp2, vp2, table2, _ = _paginate(k8.cuda(), v8.cuda(), ps, seed=2)
    assert not torch.equal(table2, table)
    kp.copy_(kp2)
    vp.copy_(vp2)
    table.copy_(table2)
    replay_and_check("graph new table")
    gks.mul_(1.5)
    gvs.mul_(0.5)
    replay_and_check("graph new scales")


# ---- 8. the automatic choice ---------------------------------------------------
def _choice():
    from torchacc_amd.ops._backend import require_extension
    ext = require_extension()
    min_keys, max_splits, limit = ext.fa_kvcache_mq_split_constants()
    return ext.fa_kvcache_mq_num_splits, min_keys, max_splits, limit


def test_automatic_choice_properties():
    choose, min_keys, max_splits, limit = _choice()
    assert min_keys >= 512 and 1 <= max_splits <= limit
    grid = [(b, hk, rows, cap, cus)
            for b in (1, 2, 8, 64) for hk in (1, 2, 8, 32)
            for rows in (1, 8, 128, 129, 2048, 16384)
            for cap in (16, 512, 1023, 1024, 2048, 4096, 16384, 1 << 20)
            for cus in (1, 64, 256, 304)]
    for b, hk, rows, cap, cus in grid:
        s = choose(b, hk, rows, cap, cus)
        tag = (b, hk, rows, cap, cus, s)
        assert 1 <= s <= max_splits, tag
        if cap < 1024:
            assert s == 1, tag
        if b * hk * -(-rows // 128) >= 2 * cus:
            assert s == 1, tag
        if s > 1:
            assert cap // s >= min_keys, tag
    # the under-filled case splits
    assert choose(1, 32, 8, 4096, 256) > 1


def test_default_call_runs_the_chosen_count():
    """cap 2048, b = 1, sq = 8, heads (8, 2): the default call is bitwise the
    call forced to the count the bound function returns, and within the
    bounds."""
    choose, *_ = _choice()
    cap, d = 2048, 128
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ns = choose(1, 2, 8 * 4, cap, cus)
    assert ns > 1, "the automatic choice should split this shape"
    c, args, kw = _device_inputs((2048,), None, 8, (8, 2), d, BF16, seed=12,
                                 cap=cap)
    forced = _call_and_check(c, args, kw, ns, BF16, d, "cap 2048 forced")
    default = _fn()(*args, return_lse=True, **kw)
    assert torch.equal(default[0], forced[0])
    assert torch.equal(default[1], forced[1])
    unsplit = _fn()(*args, return_lse=True, num_splits=1, **kw)
    _check(unsplit[0], unsplit[1], c["ref"], c["ref_lse"], BF16, d,
           "cap 2048 unsplit")


# ---- 9. argument errors --------------------------------------------------------
def test_argument_errors():
    fn = _fn()
    _, _, _, limit = _choice()
    q, k, v = _make(2, 3, 8, 2, 64, BF16, cap=128)
    gq, gk, gv = (_gpu(t, BF16) for t in (q, k, v))
    lens = _i32([5, 100]).cuda()
    for bad in (-1, 2.0, "3", None, True):
        with pytest.raises((AssertionError, TypeError)):
            fn(gq, gk, gv, lens, num_splits=bad)
    with pytest.raises(RuntimeError):          # above the documented limit
        fn(gq, gk, gv, lens, num_splits=limit + 1)
    assert torch.equal(fn(gq, gk, gv, lens, num_splits=limit),
                       fn(gq, gk, gv, lens, num_splits=2))   # 2 tiles at most
    # fp32 q is not covered by the kernel: validated, then ignored
    fq, fk, fv = (t.cuda() for t in (q, k, v))
    a = fn(fq, fk, fv, lens, num_splits=3)
    b = fn(fq, fk, fv, lens)
    assert torch.equal(a, b)
    with pytest.raises(AssertionError):
        fn(fq, fk, fv, lens, num_splits=-1)
