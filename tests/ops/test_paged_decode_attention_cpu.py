"""Paged (block-table) decode attention on the CPU reference path, the
PagedKVCache bookkeeping, and generate(page_size=) on a tiny model.

The paged reference gathers each sequence's pages and runs the contiguous
reference, so equality with the contiguous op on the gathered cache is
exact (torch.equal)."""
import pytest
import torch


def _op():
    from torchacc_amd.ops import flash_attn_with_kvcache
    return flash_attn_with_kvcache


def _make(b, cap, hq, hk, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, 1, hq, d, generator=g)
    k = torch.randn(b, cap, hk, d, generator=g)
    v = torch.randn(b, cap, hk, d, generator=g)
    return q, k, v


def _paginate(k, v, ps, extra=1, seed=1):
    """Cut contiguous [b, cap, hk, d] caches into pages placed at permuted
    physical indices. Returns pools, the table and the indices of `extra`
    spare pages that no table entry names."""
    b, cap, hk, d = k.shape
    w = cap // ps
    n = b * w + extra
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    table = perm[:b * w].view(b, w).to(torch.int32)
    kp = torch.zeros(n, ps, hk, d, dtype=k.dtype)
    vp = torch.zeros(n, ps, hk, d, dtype=v.dtype)
    kp[table.reshape(-1).long()] = k.reshape(b * w, ps, hk, d)
    vp[table.reshape(-1).long()] = v.reshape(b * w, ps, hk, d)
    return kp, vp, table, perm[b * w:]


LENS = [0, 1, 16, 17, 45]


@pytest.mark.parametrize("wl", [-1, 20])
def test_paged_reference_equals_contiguous(wl):
    """Permuted pages, lengths around the page edges; wl = 20 puts lo
    mid-page (45 - 1 - 20 = 24 = page 1, slot 8)."""
    fn = _op()
    q, k, v = _make(len(LENS), 48, 4, 2, 32)
    lens = torch.tensor(LENS, dtype=torch.int32)
    kp, vp, table, _ = _paginate(k, v, 16)
    assert not torch.equal(table.reshape(-1),
                           torch.arange(table.numel(), dtype=torch.int32))
    want = fn(q, k, v, cache_seqlens=lens, window_size=(wl, -1),
              return_lse=True)
    got = fn(q, kp, vp, cache_seqlens=lens, window_size=(wl, -1),
             return_lse=True, block_table=table)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # int64 table
    got64 = fn(q, kp, vp, cache_seqlens=lens, window_size=(wl, -1),
               block_table=table.long())
    assert torch.equal(got64, want[0])


def test_shared_prefix_pages():
    fn = _op()
    q, k, v = _make(2, 64, 4, 2, 32, seed=2)
    k[1, :32], v[1, :32] = k[0, :32], v[0, :32]     # common 2-page prefix
    lens = torch.tensor([40, 64], dtype=torch.int32)
    kp, vp, table, _ = _paginate(k, v, 16)
    table[1, :2] = table[0, :2]                     # both rows name them
    want = fn(q, k, v, cache_seqlens=lens, return_lse=True)
    got = fn(q, kp, vp, cache_seqlens=lens, return_lse=True,
             block_table=table)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("wl", [-1, 20])
def test_nan_outside_the_visible_range_cannot_matter(wl):
    fn = _op()
    q, k, v = _make(len(LENS), 48, 4, 2, 32, seed=3)
    lens = torch.tensor(LENS, dtype=torch.int32)
    want = fn(q, k, v, cache_seqlens=lens, window_size=(wl, -1),
              return_lse=True)
    nan = float("nan")
    for i, n in enumerate(LENS):
        lo = max(0, n - 1 - wl) if wl >= 0 else 0
        for t in (k, v):
            t[i, n:] = nan
            t[i, :lo] = nan
    kp, vp, table, spare = _paginate(k, v, 16)
    kp[spare[0]] = nan
    vp[spare[0]] = nan
    for i, n in enumerate(LENS):        # unused logical pages -> NaN page
        table[i, (n + 15) // 16:] = int(spare[0])
    got = fn(q, kp, vp, cache_seqlens=lens, window_size=(wl, -1),
             return_lse=True, block_table=table)
    assert bool(torch.isfinite(got[0]).all())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_unused_entries_are_clamped_not_dereferenced():
    """The gather must not raise on whatever unused entries hold."""
    fn = _op()
    q, k, v = _make(2, 32, 4, 2, 32, seed=4)
    lens = torch.tensor([5, 16], dtype=torch.int32)
    kp, vp, table, _ = _paginate(k, v, 16)
    want = fn(q, k, v, cache_seqlens=lens)
    table[:, 1] = torch.tensor([10 ** 6, -7], dtype=torch.int32)
    got = fn(q, kp, vp, cache_seqlens=lens, block_table=table)
    assert torch.equal(got, want)


def test_argument_errors():
    fn = _op()
    q, k, v = _make(2, 32, 4, 2, 32)
    lens = torch.tensor([5, 16], dtype=torch.int32)
    kp, vp, table, _ = _paginate(k, v, 16)
    with pytest.raises(AssertionError, match="requires cache_seqlens"):
        fn(q, kp, vp, block_table=table)
    with pytest.raises(AssertionError):         # wrong rank
        fn(q, kp, vp, cache_seqlens=lens, block_table=table.reshape(-1))
    with pytest.raises(AssertionError):         # wrong batch
        fn(q, kp, vp, cache_seqlens=lens, block_table=table[:1])
    with pytest.raises(AssertionError):         # float table
        fn(q, kp, vp, cache_seqlens=lens, block_table=table.float())
    with pytest.raises(AssertionError):         # another device class
        fn(q, kp, vp, cache_seqlens=lens, block_table=table.to("meta"))


def _pool(b=2, num_pages=6, ps=16, width=4):
    from torchacc_amd.models.generation import PagedKVCache
    return PagedKVCache([(2, 8), (2, 8)], b, num_pages, ps, width,
                        torch.float32, "cpu")


def test_paged_cache_reserve_free_reuse():
    pc = _pool()
    pc.reserve(0, 17)                           # 2 pages
    pc.reserve(1, 16)                           # 1 page
    assert pc.owned == [2, 1] and len(pc.free_pages) == 3
    first = pc.table_host[0, :2].tolist()
    assert torch.equal(pc.table, pc.table_host)
    pc.reserve(0, 20)                           # still 2 pages
    assert pc.owned[0] == 2
    pc.free(0)
    assert pc.owned[0] == 0 and len(pc.free_pages) == 5
    assert pc.table_host[0].tolist() == [0, 0, 0, 0]
    pc.reserve(0, 32)
    assert pc.table_host[0, :2].tolist() == first      # pages reused
    held = pc.table_host[0, :2].tolist() + pc.table_host[1, :1].tolist()
    assert len(set(held)) == 3                  # no page handed out twice
    assert torch.equal(pc.table, pc.table_host)


def test_paged_cache_exhaustion_raises():
    pc = _pool(num_pages=3)
    pc.reserve(0, 32)
    with pytest.raises(RuntimeError, match=r"exhausted.*of 3 are free"):
        pc.reserve(1, 32)
    assert pc.owned[1] == 0 and len(pc.free_pages) == 1    # nothing taken
    with pytest.raises(RuntimeError, match="block table holds 4"):
        pc.reserve(0, 65)


def test_paged_cache_slot_indices():
    pc = _pool()
    pc.reserve(1, 40)
    pc.reserve(0, 40)
    pos = torch.tensor([[0, 15, 16, 39], [1, 17, 31, 32]])
    got = pc.slot_indices(pos).view(2, 4)
    th = pc.table_host
    for i in range(2):
        for j in range(4):
            p = int(pos[i, j])
            assert int(got[i, j]) == int(th[i, p // 16]) * 16 + p % 16
    # writing through the slots lands where the gather reads
    new = torch.randn(2, 4, 2, 8)
    pc.begin_step(pos)
    layer = list(pc)[1]
    layer.write(new, -new)
    kc, vc = pc.gather(1, 40)
    for i in range(2):
        for j in range(4):
            assert torch.equal(kc[i, int(pos[i, j])], new[i, j])
            assert torch.equal(vc[i, int(pos[i, j])], -new[i, j])


@pytest.mark.parametrize("family", ["llama", "qwen2"])
def test_generate_paged_matches_default(family):
    torch.manual_seed(0)
    if family == "llama":
        from torchacc_amd.models import LlamaForCausalLM, llama_tiny
        model = LlamaForCausalLM(llama_tiny())
    else:
        from torchacc_amd.models import Qwen2ForCausalLM, qwen2_tiny
        model = Qwen2ForCausalLM(qwen2_tiny())
    model.eval()
    ids = torch.randint(0, 1024, (2, 12))
    want = model.generate(ids, max_new_tokens=8)
    got = model.generate(ids, max_new_tokens=8, page_size=16)
    assert torch.equal(got, want), (got[:, 12:], want[:, 12:])


def test_generate_returns_pages_to_a_caller_owned_pool():
    from torchacc_amd.models import LlamaForCausalLM, llama_tiny
    from torchacc_amd.models.generation import PagedKVCache
    torch.manual_seed(0)
    model = LlamaForCausalLM(llama_tiny()).eval()
    ids = torch.randint(0, 1024, (2, 12))
    want = model.generate(ids, max_new_tokens=8)
    pool = PagedKVCache.for_model(model, 2, 4, 16, 20)   # 2 pages each
    for _ in range(2):
        got = model.generate(ids, max_new_tokens=8, kv_pool=pool)
        assert torch.equal(got, want)
        assert len(pool.free_pages) == 4 and pool.owned == [0, 0]
