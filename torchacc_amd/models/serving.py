"""Continuous batching over the paged KV cache (greedy decoding).

``ContinuousBatcher`` keeps up to ``max_batch`` requests in flight on one
``PagedKVCache``. Every ``step`` is one ragged forward pass: a row that is
still inside its prompt contributes its next piece of at most
``prefill_chunk`` tokens, a decoding row contributes one token, an idle row
none. Each token sits at its own sequence's position, so the step rotates q
and k at per-token positions and writes K / V straight into the pages with
``rope_kv_cache_write`` (one launch per layer), then attends the cache in
place: ``flash_attn_with_kvcache`` when every row holds exactly one token,
``flash_attn_chunk_with_kvcache`` with ``q_seqlens`` otherwise. Every piece of
a prompt, the first included, attends the cache it has just written.

Admission is FIFO. A waiting request takes the lowest free row once the pool
has pages for its prompt plus ``max_new_tokens``; they are reserved there and
then, so a running request never waits for memory (no preemption, no swap, no
deadlock). A request at the head of the queue that does not fit yet blocks
those behind it. Pages go back when a request ends, and its row can be taken
again at the start of the next ``step``.

The step's small tensors (ids, positions, lengths) are built on the host and
copied to the device in one transfer; the only device-to-host copy of a step
is the argmax tokens.

Usage::

    eng = ContinuousBatcher(model, max_batch=8, num_pages=2048, page_size=16,
                            max_len=4096)
    rid = eng.add(prompt_ids, max_new_tokens=64, eos_token_id=2)
    outs = eng.run()          # {rid: prompt + generated tokens}
"""
from collections import deque
from typing import Optional

import torch

from ..ops.flash_attn import (flash_attn_chunk_with_kvcache,
                              flash_attn_with_kvcache, rope_kv_cache_write)
from ..ops.rmsnorm import fused_add_rms_norm
from .generation import PagedKVCache, _configure_scales, _is_fp8


class _Request:

    def __init__(self, rid, prompt, max_new_tokens, eos_token_id):
        self.rid = rid
        self.seq = prompt              # prompt + generated tokens (host ints)
        self.prompt_len = len(prompt)
        self.max_new_tokens = max_new_tokens
        self.eos_token_id = eos_token_id
        self.cached = 0                # tokens whose K / V are in the pages

    @property
    def generated(self) -> int:
        return len(self.seq) - self.prompt_len


class ContinuousBatcher:
    """See the module docstring. ``max_len`` bounds prompt + new tokens of one
    request (the block table's width); ``num_pages`` pages of ``page_size``
    tokens are shared by all rows. ``kv_dtype="fp8"`` needs ``kv_scales``
    (one ``(k_scale, v_scale)`` per layer, as in ``generate``)."""

    def __init__(self, model, max_batch: int, num_pages: int, page_size: int,
                 max_len: int, prefill_chunk: int = 64, kv_dtype=None,
                 kv_scales=None):
        assert max_batch >= 1 and prefill_chunk >= 1 and max_len >= 1
        fp8 = _is_fp8(kv_dtype)
        if fp8 and kv_scales is None:
            raise ValueError(
                "ContinuousBatcher: an fp8 KV cache needs kv_scales. The "
                "scales are per layer and kv head and shared by every "
                "request in the pool, so calibrating them from one prompt, "
                "as generate does, has no meaning here")
        if kv_scales is not None and not fp8:
            raise ValueError("kv_scales applies to an fp8 KV cache only")
        self.model = model
        self.max_batch = max_batch
        self.prefill_chunk = prefill_chunk
        self.pool = PagedKVCache.for_model(model, max_batch, num_pages,
                                           page_size, max_len,
                                           kv_dtype=kv_dtype)
        if fp8:
            _configure_scales(self.pool, kv_scales, 1.0)
        self.device = self.pool.table.device
        self.rows = [None] * max_batch     # _Request or None per batch row
        self.waiting = deque()
        self.done = {}
        self._next_rid = 0

    # ---- requests ----------------------------------------------------------
    def _pages(self, n_tokens: int) -> int:
        return (n_tokens + self.pool.page_size - 1) // self.pool.page_size

    def add(self, prompt_ids, max_new_tokens: int,
            eos_token_id: Optional[int] = None) -> int:
        """Queue a request (1-D prompt, at least one token); returns its id.
        Raises ``ValueError`` when it could never be admitted."""
        prompt = torch.as_tensor(prompt_ids)
        if prompt.dim() != 1 or prompt.numel() < 1:
            raise ValueError("ContinuousBatcher.add: the prompt must be 1-D "
                             "with at least one token")
        if max_new_tokens < 1:
            raise ValueError("ContinuousBatcher.add: max_new_tokens must be "
                             ">= 1")
        total = prompt.numel() + max_new_tokens
        limit = self.model.config.max_position_embeddings
        if total > limit:
            raise ValueError(
                f"ContinuousBatcher.add: {total} tokens exceed "
                f"max_position_embeddings={limit}")
        need = self._pages(total)
        if need > self.pool.table_width or need > self.pool.num_pages:
            raise ValueError(
                f"ContinuousBatcher.add: {total} tokens need {need} pages of "
                f"{self.pool.page_size}; the block table holds "
                f"{self.pool.table_width} per sequence and the pool "
                f"{self.pool.num_pages}")
        rid = self._next_rid
        self._next_rid += 1
        self.waiting.append(_Request(rid, prompt.tolist(), max_new_tokens,
                                     eos_token_id))
        return rid

    def idle(self) -> bool:
        return not self.waiting and all(r is None for r in self.rows)

    def _admit(self):
        while self.waiting:
            req = self.waiting[0]
            free = [i for i, r in enumerate(self.rows) if r is None]
            total = req.prompt_len + req.max_new_tokens
            if not free or self._pages(total) > len(self.pool.free_pages):
                return          # the head of the queue blocks the rest
            self.waiting.popleft()
            self.rows[free[0]] = req
            self.pool.reserve(free[0], total)

    # ---- one ragged step -----------------------------------------------------
    @torch.no_grad()
    def step(self, return_logits: bool = False):
        """Admit what fits, run one forward pass, return ``[(rid, token,
        finished), ...]`` for the rows that produced a token (rows still
        inside their prompt produce none). ``return_logits=True`` returns
        ``(events, logits)`` with the fp32 logits [len(events), vocab] in the
        order of the events."""
        self._admit()
        b = self.max_batch
        n = [0] * b
        for i, req in enumerate(self.rows):
            if req is None:
                continue
            if req.cached < req.prompt_len:
                n[i] = min(self.prefill_chunk, req.prompt_len - req.cached)
            else:
                n[i] = 1
        sq = max(n)
        if sq == 0:
            empty = torch.empty(0, self.model.config.vocab_size)
            return ([], empty) if return_logits else []
        active = [i for i in range(b) if n[i] > 0]
        # host side of the step: ids | positions | lens | n | last-row index
        tok = b * sq
        pack = torch.zeros(2 * tok + 2 * b + len(active), dtype=torch.int64)
        ids_h = pack[:tok].view(b, sq)
        pos_h = pack[tok:2 * tok].view(b, sq)
        pos_h.fill_(-1)
        lens_h = pack[2 * tok:2 * tok + b]
        n_h = pack[2 * tok + b:2 * tok + 2 * b]
        last_h = pack[2 * tok + 2 * b:]
        for r, i in enumerate(active):
            req, c = self.rows[i], self.rows[i].cached
            ids_h[i, :n[i]] = torch.tensor(req.seq[c:c + n[i]])
            pos_h[i, :n[i]] = torch.arange(c, c + n[i])
            lens_h[i] = c + n[i]
            n_h[i] = n[i]
            last_h[r] = i * sq + n[i] - 1
        dev = pack.to(self.device)
        ids = dev[:tok].view(b, sq)
        positions = dev[tok:2 * tok]
        self.pool.lens.copy_(dev[2 * tok:2 * tok + b])
        q_lens = dev[2 * tok + b:2 * tok + 2 * b]
        last = dev[2 * tok + 2 * b:]
        slots = self.pool.slot_indices_ragged(positions.view(b, sq))
        decode = sq == 1 and len(active) == b
        longest = int(lens_h.max())

        logits = self._forward(ids, positions, slots, q_lens, last, decode,
                               longest)
        tokens = logits.argmax(-1).tolist()     # the step's one D2H copy

        events, keep = [], []
        for r, i in enumerate(active):
            req = self.rows[i]
            req.cached += n[i]
            if req.cached < req.prompt_len:
                continue                        # mid-prompt: token discarded
            t = tokens[r]
            req.seq.append(t)
            finished = (req.generated >= req.max_new_tokens
                        or (req.eos_token_id is not None
                            and t == req.eos_token_id))
            if finished:
                self.done[req.rid] = torch.tensor(req.seq, dtype=torch.int64)
                self.pool.free(i)
                self.rows[i] = None
            events.append((req.rid, t, finished))
            keep.append(r)
        if return_logits:
            return events, logits[keep].float()
        return events

    def _forward(self, ids, positions, slots, q_lens, last, decode, longest):
        """ids [b, sq] -> logits [rows, vocab] of the active rows' last real
        tokens."""
        m, pool = self.model, self.pool
        b, sq = ids.shape
        delta = m.embed_tokens(ids)
        residual = None
        for layer, cache in zip(m.layers, pool):
            y1, resid = fused_add_rms_norm(
                delta, residual, layer.input_layernorm.weight,
                layer.input_layernorm.variance_epsilon)
            attn = layer.self_attn
            h, hk, hd = attn.num_heads, attn.num_kv_heads, attn.head_dim
            q = attn.q_proj(y1).view(b, sq, h, hd)
            k = attn.k_proj(y1).view(b, sq, hk, hd)
            v = attn.v_proj(y1).view(b, sq, hk, hd)
            q = rope_kv_cache_write(q, k, v, m.rope_cos, m.rope_sin,
                                    positions, cache.k, cache.v, slots,
                                    **cache.scales())
            wl = -1
            sw = getattr(getattr(attn, "cfg", None), "sliding_window", None)
            if sw is not None and longest > sw:
                wl = sw
            if decode:
                o = flash_attn_with_kvcache(
                    q, cache.k, cache.v, cache_seqlens=pool.lens,
                    window_size=(wl, -1), block_table=pool.table,
                    **cache.scales())
            else:
                o = flash_attn_chunk_with_kvcache(
                    q, cache.k, cache.v, pool.lens, q_seqlens=q_lens,
                    window_size=(wl, -1), block_table=pool.table,
                    **cache.scales())
            a = attn.o_proj(o.reshape(b, sq, h * hd))
            y2, resid2 = fused_add_rms_norm(
                a, resid, layer.post_attention_layernorm.weight,
                layer.post_attention_layernorm.variance_epsilon)
            delta = layer.mlp(y2)
            residual = resid2
        x, _ = fused_add_rms_norm(delta, residual, m.norm.weight,
                                  m.norm.variance_epsilon)
        x = x.reshape(b * sq, -1).index_select(0, last)
        return m.lm_head(x)

    def run(self):
        """Step until nothing is waiting or running; returns ``{rid: 1-D
        int64 tensor of prompt + generated tokens}`` for every request that
        has finished since the last call."""
        while not self.idle():
            self.step()
        out, self.done = self.done, {}
        return out
