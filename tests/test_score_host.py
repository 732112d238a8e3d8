"""Host side of GromaModel.score() (no GPU): the scored-row plan, evalkit.rank_choices, and the argument checks of
gr_label_logprob_rows, which reject bad calls before any launch."""
import ctypes
import math

import pytest
import torch

from groma_amd import evalkit, scoring
from groma_amd.constants import IGNORE_INDEX

IG = IGNORE_INDEX


def _spliced():
    """three ragged rows of spliced labels, right-padded with IGNORE_INDEX to L = 9, and for every expanded position the caller's
    own label index (what splicing arange(n) the same way gives; IGNORE_INDEX on the inserted image / region runs and the padding)"""
    labels = torch.tensor([
        [IG, IG, IG, IG, IG, IG, IG, IG, IG],      # row 0: nothing scored (5 real positions, the rest padding)
        [41, IG, IG, 17, IG, 23, 5, IG, IG],       # row 1: a label on position 0 (never scored), 7 real positions
        [IG, 3, IG, IG, IG, IG, IG, 8, 99],        # row 2: full length, a label on the last position
    ])
    own = torch.tensor([
        [0, 1, IG, IG, 3, IG, IG, IG, IG],
        [0, IG, IG, 2, 3, 4, 5, IG, IG],
        [0, 1, IG, IG, IG, 3, 4, 5, 6],
    ])
    return labels, own


def test_plan_matches_a_plain_loop():
    labels, own = _spliced()
    plan = scoring.score_plan(labels, own, vocab_size=100)
    rows, targets, owner, pos = [], [], [], []
    bs, L = labels.shape
    for b in range(bs):
        for p in range(1, L):                      # position 0 has nothing in front of it
            if int(labels[b, p]) != IG:
                rows.append(b * L + p - 1), targets.append(int(labels[b, p])), owner.append(b), pos.append(int(own[b, p]))
    assert plan.rows.dtype == torch.int32 and plan.targets.dtype == torch.int64
    assert plan.rows.tolist() == rows == [11, 13, 14, 18, 24, 25]
    assert plan.targets.tolist() == targets == [17, 23, 5, 3, 8, 99]
    assert plan.owner.tolist() == owner == [1, 1, 1, 2, 2, 2]
    assert plan.positions.tolist() == pos == [2, 4, 5, 1, 5, 6]
    assert plan.counts.tolist() == [0, 3, 3] and plan.counts.dtype == torch.int64
    assert 41 not in plan.targets.tolist()         # the label on position 0 is dropped
    for t in (plan.rows, plan.targets, plan.owner, plan.positions):
        assert t.is_contiguous() and t.device.type == "cpu"


def test_plan_of_nothing_and_bad_targets():
    labels, own = _spliced()
    empty = scoring.score_plan(torch.full((2, 4), IG), torch.zeros((2, 4), dtype=torch.int64), vocab_size=100)
    assert empty.rows.numel() == 0 and empty.counts.tolist() == [0, 0]
    with pytest.raises(ValueError, match="99"):
        scoring.score_plan(labels, own, vocab_size=99)              # a target == vocab_size
    neg = labels.clone()
    neg[1, 3] = -7                                                  # negative, but not IGNORE_INDEX
    with pytest.raises(ValueError):
        scoring.score_plan(neg, own, vocab_size=100)
    first = labels.clone()
    first[1, 0] = 5000                                              # position 0 is never scored, so never validated
    assert scoring.score_plan(first, own, vocab_size=100).targets.tolist() == [17, 23, 5, 3, 8, 99]
    with pytest.raises(ValueError):
        scoring.score_plan(labels, own[:, :-1], vocab_size=100)


def test_rank_choices():
    lp = torch.tensor([-6.0, -4.0, -4.0, -9.0, -1.0, 0.0, -2.5, float("nan")], dtype=torch.float64)
    nt = torch.tensor([2, 4, 1, 9, 1, 0, 1, 3])
    groups = [[0, 1, 2], [3, 4], [5, 6], [1, 2], [5], [7, 3]]
    # sums: ties (-4, -4) go to the first; a zero-token row (sum 0) never wins; a lone zero-token row answers 0; NaN ranks last
    assert evalkit.rank_choices(lp, nt, groups) == [1, 1, 1, 0, 0, 1]
    # per token: -3, -1, -4 | -1, -1 (a tie: the first) | -, -2.5 | -1, -4
    assert evalkit.rank_choices(lp, nt, groups, length_normalize=True) == [1, 0, 1, 0, 0, 1]
    assert evalkit.rank_choices(lp.tolist(), nt.tolist(), [[2, 1]]) == [0]
    with pytest.raises(ValueError):
        evalkit.rank_choices(lp, nt[:-1], groups)
    with pytest.raises(ValueError):
        evalkit.rank_choices(lp, nt, [[]])
    assert math.isnan(float(lp[7]))


def test_c_entry_rejects_bad_arguments_without_a_gpu():
    """EINVAL (22) before any launch"""
    import __graft_entry__ as g
    g.build()
    from groma_amd import _lib
    one = ctypes.c_void_p(1)  # non-null; validation only
    for prec in ("bf16", "fp16", "ref"):  # the source is built into all three libraries
        f = _lib.load(prec).gr_label_logprob_rows
        assert f(None, 4, 100, 100, one, one, None, None, None, None) == 22
        assert f(one, 4, 100, 100, None, one, None, None, None, None) == 22
        assert f(one, 4, 100, 100, one, None, None, None, None, None) == 22
        assert f(one, 0, 100, 100, one, one, None, None, None, None) == 22
        assert f(one, -1, 100, 100, one, one, None, None, None, None) == 22
        assert f(one, 4, 0, 100, one, one, None, None, None, None) == 22
        assert f(one, 4, 100, 99, one, one, None, None, None, None) == 22
        assert _lib.load(prec).gr_gather_rows_f32(None, one, one, 4, 8, 4, None) == 22
        assert _lib.load(prec).gr_gather_rows_f32(one, one, one, 4, 6, 4, None) == 22   # C % 4
