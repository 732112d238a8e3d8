"""Grounded decoding: the region-token grammar of Groma's answer format, stated on the host.

The model is trained to answer `<p>phrase</p><roi><r_k>...</roi>`, where `<r_k>` names the k-th row of the image's `pred_boxes`
(R: groma/data/datasets/refcoco_rec.py:170-173, coco.py:100-103).  `generate(grounded=True)` and `ContinuousBatcher(grounded=True)`
enforce that format inside the decode step: the device kernel gr_grammar_step (csrc/grammar.hip) writes -inf over the banned
logits between the head GEMV and the sampler.  This module is the statement of the same table in plain Python / torch -- what the
kernel is tested against, and what a caller checks an answer with.

Ids (GrammarIds.from_model): `bor` / `eor` = `<roi>` / `</roi>`; R = [r_first, r_first + r_count) = model.box_idx_token_ids, which
must be contiguous; `never` = the ids that cannot occur in an answer (`<image>`, `<region>`, `<refer_box>`, `<ground_box>`,
`<refer_feat>`, `[PAD]`; at most 8).

Every row has a state s and a box count n -- the number of `<r_k>` index ids its prompt was spliced with (the rows of `pred_boxes`
of its image), clamped to r_count.

    state      meaning                        banned ids
    -1         row not constrained            none (the row's logits are not touched)
     0  TEXT   outside a region list          all of R; eor; never; bor as well when n == 0
     1  OPEN   directly behind <roi>          everything except r_first .. r_first+n-1 (n == 0: everything except eor)
     2  BODY   behind at least one <r_k>      everything except r_first .. r_first+n-1 and eor

The transition on the last emitted token t is total: t == bor -> 1; t in R -> 2; t == eor -> 0; anything else (no token yet, a
pad, an EOS) leaves s unchanged; state -1 never changes; a row starts in state 0.

Consequences:
  * EOS is reachable only in TEXT: an answer never ends inside a region list of its own accord;
  * every `<r_k>` emitted has k < n: it names a box the image has;
  * a region list is non-empty (OPEN allows no `</roi>` while the image has boxes);
  * `max_new_tokens` may still cut a row inside a list -- the final state (Request.grammar_state, first_violation's caller) shows it.
"""
from dataclasses import dataclass
from typing import Tuple

import torch

FREE, TEXT, OPEN, BODY = -1, 0, 1, 2


@dataclass(frozen=True)
class GrammarIds:
    """the token ids the grammar speaks about"""
    bor: int
    eor: int
    r_first: int
    r_count: int
    never: Tuple[int, ...] = ()

    def __post_init__(self):
        if len(self.never) > 8:
            raise ValueError("at most 8 `never` ids")
        if self.r_count < 0 or self.r_first < 0 or self.bor == self.eor or self.in_range(self.bor) or self.in_range(self.eor):
            raise ValueError("<roi> / </roi> must be two ids outside the <r_k> range")

    def in_range(self, t):
        return self.r_first <= t < self.r_first + self.r_count

    @classmethod
    def from_model(cls, model):
        """the ids of a model behind init_special_token_id(tokenizer); ValueError when they do not describe the grammar"""
        bor, eor = getattr(model, "bor_token_id", None), getattr(model, "eor_token_id", None)
        box = list(getattr(model, "box_idx_token_ids", None) or [])
        if bor is None or eor is None or not box:
            raise ValueError("grounded decoding needs the ids of <roi>, </roi> and the <r_k>: call init_special_token_id(tokenizer)")
        if any(b != box[0] + i for i, b in enumerate(box)):
            raise ValueError("grounded decoding needs contiguous <r_k> token ids (model.box_idx_token_ids)")
        never = []
        eos = getattr(getattr(model, "generation_config", None), "eos_token_id", None)   # (a tokenizer whose pad IS the EOS: not banned)
        for name in ("img_token_id", "reg_token_id", "refer_box_token_id", "ground_box_token_id", "refer_feat_token_id", "pad_token_id"):
            t = getattr(model, name, None)
            if t is not None and int(t) not in never and (eos is None or int(t) != int(eos)):
                never.append(int(t))
        return cls(int(bor), int(eor), int(box[0]), len(box), tuple(never))


def next_state(state, token, ids):
    """the state behind emitting `token` (None: no token yet) in `state`"""
    if state < 0 or token is None:
        return state
    token = int(token)
    if token == ids.bor:
        return OPEN
    if ids.in_range(token):
        return BODY
    if token == ids.eor:
        return TEXT
    return state


def banned_mask(state, n, V, ids):
    """bool [V]: the ids a row in `state` with n boxes may not emit next"""
    n = max(0, min(int(n), ids.r_count))
    m = torch.zeros((V,), dtype=torch.bool)
    if state < 0:
        return m
    if state == TEXT:
        m[ids.r_first: ids.r_first + ids.r_count] = True
        m[ids.eor] = True
        for t in ids.never:
            m[t] = True
        if n == 0:
            m[ids.bor] = True
        return m
    m[:] = True
    m[ids.r_first: ids.r_first + n] = False
    if state == BODY or n == 0:
        m[ids.eor] = False
    return m


def first_violation(new_ids, n, ids, stop=None):
    """index of the first token of an answer (a row's new ids, read from state TEXT) that the grammar bans, or None.  Tokens behind
    the first `stop` id (an EOS: what follows is padding) are not read."""
    s = TEXT
    n = max(0, min(int(n), ids.r_count))
    for i, t in enumerate(int(x) for x in new_ids):
        if s == TEXT:
            bad = ids.in_range(t) or t == ids.eor or t in ids.never or (n == 0 and t == ids.bor)
        else:
            bad = not (ids.r_first <= t < ids.r_first + n or (t == ids.eor and (s == BODY or n == 0)))
        if bad:
            return i
        if stop is not None and t == stop:
            return None
        s = next_state(s, t, ids)
    return None


def final_state(new_ids, ids, state=TEXT):
    """the state behind a row's new ids (OPEN / BODY: max_new_tokens cut it inside a region list)"""
    for t in new_ids:
        state = next_state(state, t, ids)
    return state
