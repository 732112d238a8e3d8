"""Host side of the per-token log-probabilities (no GPU): evalkit's per-box confidence, submit()'s argument check and the
batcher's bookkeeping, which keeps one log-probability per returned token whatever ends the request."""
import math
from types import SimpleNamespace

import pytest
import torch

from groma_amd import engine, evalkit
from groma_amd.serving import ContinuousBatcher


BOX_IDS = list(range(100, 110))     # <r_0> .. <r_9>


def test_lvis_score_is_the_probability_of_the_selecting_token():
    # row 0: <r_2>, text, <r_0>, <r_2> again (the first <r_2> counts), <r_7> (no such box: dropped); row 1: no region token
    seq = torch.tensor([[1, 1, 102, 5, 100, 102, 107], [1, 1, 5, 6, 7, 8, 9]])
    lp = torch.tensor([[-0.5, -9.0, -0.25, -2.0, -7.0], [-1.0] * 5])
    boxes = [torch.tensor([[0.5, 0.5, 0.2, 0.2], [0.3, 0.3, 0.1, 0.1], [0.6, 0.4, 0.2, 0.4]]), torch.zeros((3, 4))]
    args = (seq, 2, boxes, [11, 12], [3, 4], [(100, 200), (50, 50)], BOX_IDS)
    plain = evalkit.lvis_results(*args)
    assert [d["score"] for d in plain] == [1.0, 1.0, 1.0]                     # the reference's constant (eval_lvis.py:166)
    scored = evalkit.lvis_results(*args, logprobs=lp)
    assert [d["bbox"] for d in scored] == [d["bbox"] for d in plain] and [d["image_id"] for d in scored] == [11, 11, 11]
    assert [d["score"] for d in scored] == [math.exp(-0.5), math.exp(-0.25), math.exp(-0.5)]
    # lists (a served request's `logprobs`) work like tensors; a wrong length is an error
    assert evalkit.grounded_scores(seq[0, 2:], lp[0].tolist(), 3, BOX_IDS) == [d["score"] for d in scored]
    with pytest.raises(ValueError):
        evalkit.grounded_scores(seq[0, 2:], [0.0], 3, BOX_IDS)


def test_rec_meter_records_the_first_box_confidence_and_keeps_its_counters():
    seq = torch.tensor([[1, 103, 101], [1, 5, 6]])
    lp = torch.tensor([[-0.125, -3.0], [-1.0, -1.0]])
    boxes = [torch.tensor([[0.5, 0.5, 0.2, 0.2]] * 4), torch.zeros((2, 4))]
    gts = [torch.tensor([[0.5, 0.5, 0.2, 0.2]]), torch.tensor([[0.5, 0.5, 0.2, 0.2]])]
    a, b = evalkit.RecMeter(), evalkit.RecMeter()
    a.update(seq, 1, boxes, gts, BOX_IDS)
    b.update(seq, 1, boxes, gts, BOX_IDS, logprobs=lp)
    assert a.summary() == b.summary() and a.scores == []
    assert len(b.scores) == 1 and b.scores[0][0] == math.exp(-0.125) and abs(b.scores[0][1] - 1.0) < 1e-6


class _LLM:
    H, hd, T, w = 2, 32, 16, {"layers": [None, None]}

    def __init__(self):
        self.graphs = engine.GraphPool()

    def new_cache(self, bs, smax, device):
        return engine.KVCache(2, bs, self.H, self.hd, smax, device)


def _batcher(rows=2):
    """a ContinuousBatcher over a model stand-in on the CPU (the one tests/test_host_logic.py grows an arena with): host logic only"""
    model = SimpleNamespace(device=torch.device("cpu"), fp8=False, precision="bf16", llm=_LLM(), vit=SimpleNamespace(G=8),
                            config=SimpleNamespace(max_region_num=5), generation_config=SimpleNamespace(eos_token_id=2))
    return ContinuousBatcher(model, max_rows=rows, max_len=64, use_graph=False)


def test_submit_checks_logprobs():
    b = _batcher()
    ids = torch.zeros(4, dtype=torch.int64)
    for bad in (9, -1, 2.5, True):
        with pytest.raises(ValueError):
            b.submit(ids, None, logprobs=bad)
    assert not b.queue and not b.live                                         # a refused call leaves nothing behind
    r = b.live[b.submit(ids, None)]
    assert r.logprobs_k is None and r.logprobs is None and r.top_logprobs is None
    r = b.live[b.submit(ids, None, logprobs=0)]
    assert r.logprobs_k == 0 and r.logprobs == [] and r.top_logprobs is None
    r = b.live[b.submit(ids, None, logprobs=8)]
    assert r.logprobs_k == 8 and r.logprobs == [] and r.top_logprobs == []
    assert int(b.lp_k.min()) == -1 and b.lp.shape == (2,) and b.top_ids.shape == (2, 8) and b.top_lp.shape == (2, 8)


@pytest.mark.parametrize("ending", ["eos", "stop", "max_new_tokens"])
@pytest.mark.parametrize("k", [0, 3])
def test_tokens_and_logprobs_stay_aligned_through_every_ending(ending, k):
    """_place's first token and the ticks' tokens go through one _emit: a request ends on EOS, on its stop id or at max_new_tokens with
    exactly one log-probability (and one list of k alternatives) per token, and its row stops asking"""
    b = _batcher()
    ids = torch.zeros(4, dtype=torch.int64)
    rid = b.submit(ids, None, max_new_tokens=4, eos_token_id=2, stop_token_id=7, logprobs=k)
    quiet = b.submit(ids, None, max_new_tokens=6, eos_token_id=2)             # a neighbour that does not ask
    r, q = b.live[rid], b.live[quiet]
    b.queue.clear()
    for x in (r, q):
        x.prompt_len = 10
    r._first_lp = (-0.5, list(range(8)), [-0.5 - j for j in range(8)])
    b._place([r, q], [(r, 0, 11, 0.0), (q, 1, 12, 0.0)])
    assert r.tokens == [11] and r.logprobs == [-0.5] and q.logprobs is None and not hasattr(r, "_first_lp")
    assert b.lp_k.tolist() == [k, -1]
    last = {"eos": 2, "stop": 7, "max_new_tokens": 13}[ending]
    stream = [12, last] if ending != "max_new_tokens" else [12, 13, 14]
    for n, t in enumerate(stream):
        lp = (-1.0 - n, [t] + list(range(7)), [-1.0 - n - j for j in range(8)])
        b._emit(r, t, lp)
        b._emit(q, 20 + n, None)
    assert r.done and not q.done and r.tokens == [11] + stream
    assert len(r.logprobs) == len(r.tokens) and r.logprobs[1:] == [-1.0 - n for n in range(len(stream))]
    if k:
        assert len(r.top_logprobs) == len(r.tokens) and all(len(t) == k for t in r.top_logprobs)
        assert r.top_logprobs[1] == [(12, -1.0), (0, -2.0), (1, -3.0)]
    else:
        assert r.top_logprobs is None
    assert b.lp_k.tolist() == [-1, -1] and q.logprobs is None and len(q.tokens) == 1 + len(stream)


def test_generate_stream_carries_logprobs():
    """generate_stream(logprobs=k) yields (ids, logprobs, top_logprobs), aligned; without it, the ids alone as before"""
    for k in (None, 0, 2):
        b = _batcher(rows=1)
        feed = iter(range(30, 40))

        def step():
            r = next(iter(b.live.values()))
            if not r.tokens:
                b.queue.clear()
            t = next(feed)
            b._emit(r, t, None if k is None else (-float(t), [t, t + 1] + [0] * 6, [-float(t), -float(t) - 1] + [0.0] * 6))
        b.step = step
        chunks = list(b.generate_stream(torch.zeros(4, dtype=torch.int64), None, max_new_tokens=3, eos_token_id=None,
                                        **({} if k is None else {"logprobs": k})))
        assert len(chunks) == 3
        if k is None:
            assert chunks[-1] == [30, 31, 32]
            continue
        ids, lps, top = chunks[-1]
        assert ids == [30, 31, 32] and lps == [-30.0, -31.0, -32.0]
        assert top is None if k == 0 else top == [[(t, -float(t)), (t + 1, -float(t) - 1)] for t in ids]


def test_sampler_entry_rejects_bad_arguments():
    """gr_sample_rows_lp validates before any launch: EINVAL (22) on a null required pointer, a non-positive size, ld < V, a top-k
    width outside 0..8 or without its arrays, a scores arena without capacity, a step-indexed arena without the step"""
    from groma_amd import _lib
    lib = _lib.load()
    P = 1   # any non-null address
    ok = [P, P, P, 4, 100, 100, None, None, None, 0, 0, None, 0, None, None, None, None, 0, 0, None]
    for i, v in ((0, None), (1, None), (2, None), (3, 0), (4, 0), (5, 99), (9, -1), (12, 9), (12, -1), (12, 8), (18, 2), (18, -1), (17, 0)):
        a = list(ok)
        a[i] = v
        if i == 17:
            a[15] = P          # scores without capacity
        assert lib.gr_sample_rows_lp(*a) == 22, (i, v)
