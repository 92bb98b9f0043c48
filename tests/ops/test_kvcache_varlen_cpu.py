"""CPU path of flash_attn_varlen_with_kvcache against a plain per-sequence
fp64 softmax loop (fp32 inputs), and PagedKVCache.slot_indices_packed against
slot_indices_ragged on the padded equivalent.

Tolerance 1e-5 absolute on out and lse; measured maximum 5.0e-7."""
import math

import pytest
import torch

from torchacc_amd.models.generation import PagedKVCache
from torchacc_amd.ops import flash_attn_varlen_with_kvcache

CAP = 64
N = [1, 0, 33, 5, 32, 64, 0, 5]
L = [30, 17, 57, 5, 64, 64, 0, 3]


def _loop_reference(q, k, v, n, lens, scale, wl):
    hq, hk = q.shape[1], k.shape[2]
    out = torch.zeros(q.shape, dtype=torch.float64)
    lse = torch.full((hq, q.shape[0]), float("-inf"), dtype=torch.float64)
    t = 0
    for i, (ni, li) in enumerate(zip(n, lens)):
        for j in range(ni):
            p = li - ni + j
            lo = max(0, p - wl) if wl >= 0 else 0
            for h in range(hq) if p >= 0 else ():
                kh = h // (hq // hk)
                s = (k[i, lo:p + 1, kh].double() @ q[t + j, h].double()) * scale
                lse[h, t + j] = torch.logsumexp(s, 0)
                out[t + j, h] = torch.softmax(s, 0) @ v[i, lo:p + 1, kh].double()
        t += ni
    return out, lse


@pytest.mark.parametrize("wl", [-1, 10])
@pytest.mark.parametrize("paged", [False, True])
def test_cpu_path_against_fp64_loop(paged, wl):
    g = torch.Generator().manual_seed(0)
    b, T, hq, hk, d = len(N), sum(N), 4, 2, 16
    q = torch.randn(T + 3, hq, d, generator=g)      # 3 rows past cu[b]
    k = torch.randn(b, CAP, hk, d, generator=g)
    v = torch.randn(b, CAP, hk, d, generator=g)
    cu = torch.tensor([0] + torch.tensor(N).cumsum(0).tolist())
    kw = {}
    kc, vc = k, v
    if paged:       # page p of sequence i at physical page (b - 1 - i) * 4 + p
        table = (torch.arange(b).flip(0).view(b, 1) * 4
                 + torch.arange(4).view(1, 4)).int()
        kc = torch.zeros(b * 4, 16, hk, d)
        vc = torch.zeros(b * 4, 16, hk, d)
        kc[table.reshape(-1).long()] = k.view(b * 4, 16, hk, d)
        vc[table.reshape(-1).long()] = v.view(b * 4, 16, hk, d)
        kw["block_table"] = table
    scale = 1.0 / math.sqrt(d)
    out, lse = flash_attn_varlen_with_kvcache(
        q, kc, vc, torch.tensor(L), cu, window_size=(wl, -1), return_lse=True,
        **kw)
    want, want_lse = _loop_reference(q[:T], k, v, N, L, scale, wl)
    assert out.shape == q.shape and lse.shape == (hq, T + 3)
    empty = torch.isinf(want_lse)
    assert torch.equal(torch.isinf(lse[:, :T]) & (lse[:, :T] < 0), empty)
    err = float((out[:T].double() - want).abs().max())
    lerr = float((lse[:, :T].double() - want_lse)[~empty].abs().max())
    print(f"cpu varlen paged={paged} wl={wl}: out {err:.2e} lse {lerr:.2e}")
    assert err <= 1e-5 and lerr <= 1e-5
    # the torch path's rows past cu[b]: zeros, lse = -inf
    assert bool((out[T:] == 0).all()) and bool(torch.isinf(lse[:, T:]).all())


def test_slot_indices_packed_equals_ragged():
    pool = PagedKVCache([(2, 8)], 3, 12, 16, 4, torch.float32, "cpu")
    for i, n_tok in enumerate((40, 64, 17)):
        pool.reserve(i, n_tok)
    n, start = [5, 0, 3], [35, 0, 14]
    sq = max(n)
    padded = torch.full((3, sq), -1)
    pos, seq = [], []
    for i, (ni, s) in enumerate(zip(n, start)):
        padded[i, :ni] = torch.arange(s, s + ni)
        pos += list(range(s, s + ni))
        seq += [i] * ni
    pos += [-1, 64, 5]            # padding, past the capacity, bad sequence id
    seq += [0, 1, 7]
    got = pool.slot_indices_packed(torch.tensor(pos), torch.tensor(seq))
    want = pool.slot_indices_ragged(padded).view(3, sq)
    want = torch.cat([want[i, :ni] for i, ni in enumerate(n)])
    assert got.dtype == torch.int64
    assert torch.equal(got[:8], want) and got[8:10].tolist() == [-1, -1]
    assert int(got[10]) == int(pool.slot_indices_ragged(
        torch.tensor([[-1], [-1], [5]]))[2])      # id clamped to the last row
