"""rope_kv_cache_write on the GPU: bitwise against the composition of the
existing ops (apply_rotary_pos_emb, then index_copy_ or kv_cache_write_fp8)
on the same inputs. Whole caches are compared as integers, which also proves
that no other slot was touched; they start from random bytes, NaN patterns
included."""
import ctypes

import pytest
import torch

from torchacc_amd.ops import (apply_rotary_pos_emb, kv_cache_write_fp8,
                              rope_kv_cache_write)
from torchacc_amd.ops.rope import build_rope_cache

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
P = 64                      # table rows
CAP, PAGE, PAGES, PITCH = 32, 16, 12, 24
# ragged starts per batch row; start + 17 <= 32 keeps every position inside
# the contiguous capacity and two table pages
STARTS = (3, 0, 11)
SHAPES = ((1, 1), (3, 1), (2, 5), (3, 17))


def _bits(t):
    return t.view(torch.uint8 if t.element_size() == 1 else torch.int16)


def _random_bytes(shape, dtype, gen):
    n = torch.empty(shape, dtype=dtype).numel() * torch.empty(
        (), dtype=dtype).element_size()
    raw = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=gen)
    return raw.cuda().view(dtype).view(shape)


class _Layout:
    """Two equal cache pairs (for the op and for the composition) plus the
    slot of every (row, position). ``store`` is what gets compared: for the
    strided pool the whole backing buffer, gaps included."""

    def __init__(self, kind, b, hk, d, cdtype, gen):
        self.kind = kind
        if kind == "contiguous":
            shape = (b, CAP, hk, d)
        elif kind == "paged":
            shape = (PAGES, PAGE, hk, d)
        else:                                   # strided pool view
            shape = (PAGES, PITCH, hk, d)
        self.store = [_random_bytes(shape, cdtype, gen) for _ in range(2)]
        self.store_ref = [t.clone() for t in self.store]
        cut = (lambda t: t[:, :PAGE]) if kind == "strided" else (lambda t: t)
        self.caches = [cut(t) for t in self.store]
        self.caches_ref = [cut(t) for t in self.store_ref]
        if kind != "contiguous":
            perm = torch.randperm(PAGES, generator=gen)
            self.table = perm[:b * 2].view(b, 2)

    def slots(self, pos):
        """positions [b, s] (host) -> flat slots [b * s] (host int64)."""
        b = pos.shape[0]
        if self.kind == "contiguous":
            return (torch.arange(b).view(b, 1) * CAP + pos).reshape(-1)
        page = self.table.gather(1, pos // PAGE)
        return (page * PAGE + pos % PAGE).reshape(-1)

    def store_slots(self, slots):
        """flat slots of the cache view -> rows of the flattened store."""
        if self.kind == "strided":
            return (slots // PAGE) * PITCH + slots % PAGE
        return slots


def _compose(q, k, v, cos, sin, pos, lay, slots, scales, ok=None):
    """The composition on the reference caches; returns q_rot. ``pos`` [b, s]
    holds consecutive positions per row. ``ok`` masks the tokens whose K / V
    are written."""
    b, s = pos.shape
    q_rot, k_rot = torch.empty_like(q), torch.empty_like(k)
    for i in range(b):
        p0 = int(pos[i, 0])
        qi, ki = apply_rotary_pos_emb(q[i:i + 1], k[i:i + 1],
                                      cos[p0:p0 + s], sin[p0:p0 + s])
        q_rot[i], k_rot[i] = qi[0], ki[0]
    _write(k_rot, v, lay, slots, scales, ok)
    return q_rot


def _write(k_rot, v, lay, slots, scales, ok=None):
    kc, vc = lay.caches_ref
    dev_slots = slots.cuda()
    if ok is not None:
        dev_slots = torch.where(ok.cuda(), dev_slots,
                                torch.full_like(dev_slots, -1))
    if scales:
        kv_cache_write_fp8(k_rot.contiguous(), v.contiguous(), kc, vc,
                           dev_slots, *scales)
        return
    rows = lay.store_slots(slots)
    keep = torch.ones_like(rows, dtype=torch.bool) if ok is None else ok
    for store, new in zip(lay.store_ref, (k_rot, v)):
        flat = store.view(-1, *store.shape[2:])
        flat.index_copy_(0, rows[keep].cuda(),
                         new.reshape(-1, *new.shape[2:])[keep.cuda()])


def _scales(hk, fp8):
    if not fp8:
        return ()
    return (torch.linspace(0.01, 0.03, hk).cuda(),
            torch.linspace(0.02, 0.05, hk).cuda())


def _assert_same(got_q, want_q, lay):
    assert got_q.dtype == want_q.dtype and got_q.shape == want_q.shape
    assert got_q.is_contiguous()
    assert torch.equal(_bits(got_q), _bits(want_q))
    for got, want in zip(lay.store, lay.store_ref):
        assert torch.equal(_bits(got), _bits(want))


def _inputs(b, s, hq, hk, d, dtype, gen):
    mk = lambda h: (torch.randn(b, s, h, d, generator=gen) * 2).to(dtype).cuda()
    return mk(hq), mk(hk), mk(hk)


@pytest.fixture(scope="module")
def tables():
    out = {}
    for d in (64, 128):
        cos, sin = build_rope_cache(P, d)
        out[d] = (cos.cuda(), sin.cuda())
    return out


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kvfp8"])
@pytest.mark.parametrize("kind", ["contiguous", "paged", "strided"])
@pytest.mark.parametrize("hq,hk", [(4, 1), (8, 2), (2, 2)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
def test_bitwise_against_composition(tables, dtype, d, hq, hk, kind, fp8):
    cos, sin = tables[d]
    gen = torch.Generator().manual_seed(hq * 1000 + d + (7 if fp8 else 0))
    scales = _scales(hk, fp8)
    for b, s in SHAPES:
        for idx in (torch.int32, torch.int64):
            q, k, v = _inputs(b, s, hq, hk, d, dtype, gen)
            lay = _Layout(kind, b, hk, d, FP8 if fp8 else dtype, gen)
            pos = torch.tensor([[STARTS[i] + j for j in range(s)]
                                for i in range(b)])
            slots = lay.slots(pos)
            want_q = _compose(q, k, v, cos, sin, pos, lay, slots, scales)
            before = lay.store[0].clone()
            got_q = rope_kv_cache_write(
                q, k, v, cos, sin, pos.reshape(-1).to(idx).cuda(),
                lay.caches[0], lay.caches[1], slots.to(idx).cuda(), *scales)
            _assert_same(got_q, want_q, lay)
            assert not torch.equal(_bits(lay.store[0]), _bits(before))


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kvfp8"])
@pytest.mark.parametrize("kind", ["contiguous", "strided"])
def test_padding_and_out_of_range_slots(tables, kind, fp8):
    """positions -1 and >= P are padding (zero q rows, nothing written);
    slots -1 and >= n0 * n1 write nothing. The composition rotates the
    tokens flattened into one sequence with their own table rows."""
    b, s, hq, hk, d, dtype = 3, 5, 8, 2, 128, torch.bfloat16
    cos, sin = tables[d]
    gen = torch.Generator().manual_seed(11)
    scales = _scales(hk, fp8)
    q, k, v = _inputs(b, s, hq, hk, d, dtype, gen)
    lay = _Layout(kind, b, hk, d, FP8 if fp8 else dtype, gen)
    pos = torch.tensor([[STARTS[i] + j for j in range(s)] for i in range(b)])
    slots = lay.slots(pos)
    pos[0, 4], pos[1, 0] = -1, P + 3
    n_slots = lay.caches[0].shape[0] * lay.caches[0].shape[1]
    slots = slots.clone()
    slots[1 * s + 2], slots[2 * s + 3] = -1, n_slots
    flat = pos.reshape(-1)
    real = (flat >= 0) & (flat < P)
    ok = real & (slots >= 0) & (slots < n_slots)
    assert int(real.sum()) == b * s - 2 and int(ok.sum()) == b * s - 4
    row = flat.clamp(0, P - 1).cuda()
    qf, kf = apply_rotary_pos_emb(q.view(1, b * s, hq, d),
                                  k.view(1, b * s, hk, d), cos[row], sin[row])
    want_q = torch.where(real.cuda().view(b, s, 1, 1), qf.view(b, s, hq, d),
                         torch.zeros_like(q))
    _write(kf.view(b, s, hk, d), v, lay, slots.clamp(0, n_slots - 1),
           scales, ok)
    got_q = rope_kv_cache_write(q, k, v, cos, sin, flat.cuda(),
                                lay.caches[0], lay.caches[1], slots.cuda(),
                                *scales)
    _assert_same(got_q, want_q, lay)
    assert int(_bits(got_q[0, 4]).abs().max()) == 0
    assert int(_bits(got_q[1, 0]).abs().max()) == 0


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kvfp8"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
def test_strided_inputs_from_one_qkv_buffer(tables, dtype, fp8):
    b, s, hq, hk, d = 2, 5, 8, 2, 64
    cos, sin = tables[d]
    gen = torch.Generator().manual_seed(13)
    scales = _scales(hk, fp8)
    qkv = torch.randn(b, s, (hq + 2 * hk) * d, generator=gen).to(dtype).cuda()
    q = qkv[..., :hq * d].view(b, s, hq, d)
    k = qkv[..., hq * d:(hq + hk) * d].view(b, s, hk, d)
    v = qkv[..., (hq + hk) * d:].view(b, s, hk, d)
    assert not q.is_contiguous() and not k.is_contiguous()
    lay = _Layout("paged", b, hk, d, FP8 if fp8 else dtype, gen)
    pos = torch.tensor([[STARTS[i] + j for j in range(s)] for i in range(b)])
    slots = lay.slots(pos)
    want_q = _compose(q, k, v, cos, sin, pos, lay, slots, scales)
    got_q = rope_kv_cache_write(q, k, v, cos, sin, pos.reshape(-1).cuda(),
                                lay.caches[0], lay.caches[1], slots.cuda(),
                                *scales)
    _assert_same(got_q, want_q, lay)


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kvfp8"])
def test_poisoned_cache_stays_bit_identical(tables, fp8):
    """Every slot starts as a NaN pattern; the unnamed ones keep it."""
    b, s, hq, hk, d, dtype = 3, 17, 4, 1, 128, torch.bfloat16
    cos, sin = tables[d]
    gen = torch.Generator().manual_seed(17)
    scales = _scales(hk, fp8)
    q, k, v = _inputs(b, s, hq, hk, d, dtype, gen)
    lay = _Layout("strided", b, hk, d, FP8 if fp8 else dtype, gen)
    for t in lay.store + lay.store_ref:
        _bits(t).fill_(0x7F if fp8 else 0x7FC1)
    assert bool(lay.store[0].float().isnan().all())
    pos = torch.tensor([[STARTS[i] + j for j in range(s)] for i in range(b)])
    slots = lay.slots(pos)
    want_q = _compose(q, k, v, cos, sin, pos, lay, slots, scales)
    got_q = rope_kv_cache_write(q, k, v, cos, sin, pos.reshape(-1).cuda(),
                                lay.caches[0], lay.caches[1], slots.cuda(),
                                *scales)
    _assert_same(got_q, want_q, lay)
    named = torch.zeros(PAGES * PITCH, dtype=torch.bool)
    named[lay.store_slots(slots)] = True
    for store in lay.store:
        nan_rows = store.float().isnan().all(-1).all(-1).reshape(-1).cpu()
        assert torch.equal(nan_rows, ~named)


def _kernel_nodes(graph):
    """(number of nodes, number of kernel nodes) of a captured graph."""
    hip = ctypes.CDLL("libamdhip64.so")
    raw = ctypes.c_void_p(graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) == 0
    kernels = 0
    for node in nodes:
        kind = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(node),
                                       ctypes.byref(kind)) == 0
        kernels += kind.value == 0          # hipGraphNodeTypeKernel
    return n.value, kernels


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kvfp8"])
def test_graph_capture_reads_indices_at_replay(tables, fp8):
    b, s, hq, hk, d, dtype = 3, 5, 8, 2, 128, torch.bfloat16
    cos, sin = tables[d]
    gen = torch.Generator().manual_seed(19)
    scales = _scales(hk, fp8)
    q, k, v = _inputs(b, s, hq, hk, d, dtype, gen)
    lay = _Layout("paged", b, hk, d, FP8 if fp8 else dtype, gen)
    pos = torch.tensor([[STARTS[i] + j for j in range(s)] for i in range(b)])
    pos2 = pos.flip(0) + 9
    pos2[1, 3] = -1
    slots, slots2 = lay.slots(pos), lay.slots(pos2.clamp_min(0))
    dev_pos, dev_slots = pos.reshape(-1).cuda(), slots.cuda()

    def call(caches, p, t):
        return rope_kv_cache_write(q, k, v, cos, sin, p, caches[0],
                                   caches[1], t, *scales)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(lay.caches, dev_pos, dev_slots)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        out = call(lay.caches, dev_pos, dev_slots)
    assert _kernel_nodes(graph) == (1, 1)
    # the eager call on the new values, on caches in the same state
    for mine, ref in zip(lay.store, lay.store_ref):
        ref.copy_(mine)
    want_q = call(lay.caches_ref, pos2.reshape(-1).cuda(), slots2.cuda())
    dev_pos.copy_(pos2.reshape(-1))
    dev_slots.copy_(slots2)
    graph.replay()
    torch.cuda.synchronize()
    _assert_same(out, want_q, lay)
    assert int(_bits(out[1, 3]).abs().max()) == 0
    # and the new values differ from the captured ones in what they write
    assert not torch.equal(slots, slots2)


def test_host_checks_name_the_op(tables):
    """What the Python front end cannot see is refused by the extension."""
    b, s, hq, hk, d, dtype = 2, 5, 4, 1, 64, torch.bfloat16
    cos, sin = tables[d]
    gen = torch.Generator().manual_seed(23)
    q, k, v = _inputs(b, s, hq, hk, d, dtype, gen)
    lay = _Layout("contiguous", b, hk, d, dtype, gen)
    pos = torch.arange(b * s).cuda()
    slots = torch.arange(b * s).cuda()
    kc, vc = lay.caches
    before = [t.clone() for t in lay.store]
    # 8 bytes past a 16-byte boundary
    q_off = torch.zeros(q.numel() + 8, dtype=dtype,
                        device="cuda")[4:4 + q.numel()].view(q.shape)
    with pytest.raises(RuntimeError, match="rope_kv_cache_write: q rows"):
        rope_kv_cache_write(q_off, k, v, cos, sin, pos, kc, vc, slots)
    cos_t = cos.t().contiguous().t()        # right shape, column-major
    with pytest.raises(RuntimeError, match="rope_kv_cache_write: cos and"):
        rope_kv_cache_write(q, k, v, cos_t, sin, pos, kc, vc, slots)
    kc_gap = torch.zeros(b, CAP, hk, d + 8, dtype=dtype,
                         device="cuda")[..., :d]
    with pytest.raises(RuntimeError,
                       match="rope_kv_cache_write: k_cache needs dense"):
        rope_kv_cache_write(q, k, v, cos, sin, pos, kc_gap, vc, slots)
    torch.cuda.synchronize()
    for got, want in zip(lay.store, before):
        assert torch.equal(_bits(got), _bits(want))
