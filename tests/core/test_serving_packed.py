"""ContinuousBatcher(packed=True) on the GPU: the bf16 case of test_serving.py
(same model, prompts, seeds, reference and bound: twice the pre-engine path's
error + 1e-3 on the logits), with mixed steps on the packed layout.

Measured (max |dlogit|): pre-engine path 0.0234, bound 0.0479, packed
engine 0.0195."""
import pytest
import torch

from tests.core.test_serving import (MAX_BATCH, NEW, NUM_PAGES, _parent_logits,
                                     _reference_logits, _run_engine, _setup)

pytestmark = pytest.mark.gpu


def test_packed_logits_within_bound_and_pages_back():
    model, prompts = _setup()
    outs, logits, eng = _run_engine(model, prompts, packed=True)
    parent_err = engine_err = 0.0
    for rid, p in enumerate(prompts):
        ref = _reference_logits(model, outs[rid], len(p))
        par = _parent_logits(model, outs[rid], len(p))
        assert ref.shape == logits[rid].shape == (NEW, 1024)
        parent_err = max(parent_err, float((par - ref).abs().max()))
        engine_err = max(engine_err,
                         float((logits[rid].cuda() - ref).abs().max()))
    bound = 2.0 * parent_err + 1e-3
    print(f"\npacked: parent max |dlogit| {parent_err:.5f}  bound {bound:.5f}  "
          f"engine max |dlogit| {engine_err:.5f}")
    assert engine_err <= bound, (engine_err, bound)
    assert len(eng.pool.free_pages) == NUM_PAGES
    assert eng.pool.owned == [0] * MAX_BATCH and eng.idle()
