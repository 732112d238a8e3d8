"""REC / LVIS evaluation post-processing for batched, image-sharded runs.

The reference's eval scripts (groma/eval/eval_rec.py:89-131, eval_lvis.py:134-168) call `model.generate` one image at
a time, pick the `<r_k>` ids out of the new tokens, look the k-th selected box up in
`outputs.hidden_states[0][-1]['pred_boxes'][0]`, and score it (REC: IoU of the FIRST grounded box against the best-matching
ground-truth box, accuracy at a threshold, mean IoU, 'missing' count, three scalar `reduce`s at the end; LVIS: xywh boxes
scaled to the image size).  Those scripts run unchanged on `groma_amd.groma.GromaModel` (same attributes and outputs).
This module is the same bookkeeping for a *batch* of images per GPU -- what the MI355X path is efficient at -- with one
all-reduce of the three counters over RCCL.  Box maths is a few dozen floats per image: host side, as in the reference.
"""
import math

import torch


def cxcywh_to_xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)


def pairwise_iou(a, b):
    """torchvision.ops.box_iou semantics on xyxy boxes"""
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = torch.max(a[:, None, :2], b[None, :, :2])
    rb = torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area_a[:, None] + area_b[None, :] - inter)


def _grounded(new_ids, n_boxes, box_idx_token_ids):
    """[(position in new_ids, k)] of the tokens <r_k> with k < n_boxes, in generation order"""
    first = box_idx_token_ids[0]
    n_tok = len(box_idx_token_ids)
    ks = [int(t) - first for t in new_ids.tolist()]
    if box_idx_token_ids != list(range(first, first + n_tok)):  # non-contiguous vocabulary: generic lookup
        table = {t: i for i, t in enumerate(box_idx_token_ids)}
        ks = [table.get(int(t), -1) for t in new_ids.tolist()]
    return [(j, k) for j, k in enumerate(ks) if 0 <= k < n_tok and k < n_boxes]


def grounded_boxes(new_ids, pred_boxes, box_idx_token_ids):
    """new_ids: generated ids of ONE image; pred_boxes [N,4] cxcywh in the order <r_j> indexes.  Returns the boxes the
    answer points at, in generation order; ids that are not <r_k>, or k >= N, are dropped (eval_rec.py:106-108)."""
    ks = [k for _, k in _grounded(new_ids, pred_boxes.shape[0], box_idx_token_ids)]
    return pred_boxes[ks] if ks else pred_boxes[:0]


def grounded_scores(new_ids, logprobs, n_boxes, box_idx_token_ids):
    """One confidence per box grounded_boxes returns, in the same order: exp(log-probability) of the region token that selected the
    box (`logprobs`: one natural-log probability per entry of new_ids -- GenerateOutput.logprobs[i] or a served request's
    `logprobs`).  A box selected by several tokens takes the FIRST one's value every time it appears."""
    lp = [float(x) for x in (logprobs.tolist() if hasattr(logprobs, "tolist") else logprobs)]
    if len(lp) != len(new_ids):
        raise ValueError("logprobs must hold one entry per generated token")
    first_lp = {}
    sel = _grounded(new_ids, n_boxes, box_idx_token_ids)
    for j, k in sel:
        first_lp.setdefault(k, lp[j])
    return [math.exp(first_lp[k]) for _, k in sel]


def region_lists(new_ids, box_idx_token_ids, bor, eor):
    """The `[k, ...]` lists of an answer, one per `<roi>...</roi>` group in generation order: the indices k of the `<r_k>` between a
    `bor` and the next `eor`.  A group that the answer's end cuts open is returned as it stands (its list may be empty); `<r_k>`
    outside a group, and ids that are neither, are skipped.  Under grounded decoding (grammar.py) every list is non-empty, every k
    is below the image's box count, and only the last one can be open."""
    table = {int(t): i for i, t in enumerate(box_idx_token_ids)}
    out, cur = [], None
    for t in (new_ids.tolist() if hasattr(new_ids, "tolist") else new_ids):
        t = int(t)
        if t == bor:
            if cur is not None:
                out.append(cur)
            cur = []
        elif t == eor:
            if cur is not None:
                out.append(cur)
            cur = None
        elif cur is not None and t in table:
            cur.append(table[t])
    if cur is not None:
        out.append(cur)
    return out


def rank_choices(sequence_logprob, num_tokens, groups, length_normalize=False):
    """Likelihood ranking of candidate answers (multiple choice): sequence_logprob / num_tokens are ScoreOutput's per-row values,
    groups a list of lists of row indices (the candidates of one question).  Returns, per group, the position INSIDE the group of
    the candidate with the largest summed log-probability -- per scored token with length_normalize.  Ties go to the first
    candidate.  A candidate with no scored token (its sum of 0 would beat every real answer) or a NaN score ranks as -inf; a group
    of nothing else answers 0.  Host only."""
    lp = [float(x) for x in (sequence_logprob.tolist() if hasattr(sequence_logprob, "tolist") else sequence_logprob)]
    nt = [int(x) for x in (num_tokens.tolist() if hasattr(num_tokens, "tolist") else num_tokens)]
    if len(lp) != len(nt):
        raise ValueError("sequence_logprob and num_tokens need one entry per row")
    picks = []
    for g in groups:
        if len(g) == 0:
            raise ValueError("a group needs at least one candidate row")
        best, best_v = 0, -math.inf
        for j, r in enumerate(g):
            v = -math.inf if nt[r] <= 0 or lp[r] != lp[r] else (lp[r] / nt[r] if length_normalize else lp[r])
            if v > best_v:
                best, best_v = j, v
        picks.append(best)
    return picks


class RecMeter:
    """Running REC counters of eval_rec.py:85-87,110-124; `summary` all-reduces them when a process group is up.  Answers generated
    with grounded=True (grammar.py) name only boxes the image has, so grounded_boxes drops no id of theirs."""

    def __init__(self, threshold=0.5):
        self.threshold = threshold
        self.m_iou = 0.0
        self.hits = 0.0
        self.invalid = 0.0
        self.count = 0.0
        self.scores = []   # with logprobs: (confidence, IoU) of every image's recorded (first grounded) box; local to this process

    def update(self, sequences, prompt_len, pred_boxes_list, gt_boxes_list, box_idx_token_ids, logprobs=None):
        """sequences [bs, P+new] (GenerateOutput.sequences); pred_boxes_list / gt_boxes_list: per-image cxcywh boxes.
        logprobs [bs, new] (GenerateOutput.logprobs, optional): the box the meter scores is recorded in `scores` with the confidence
        exp(log-probability of its region token); the counters do not depend on it."""
        for i in range(sequences.shape[0]):
            self.count += 1
            sel = grounded_boxes(sequences[i, prompt_len:].cpu(), pred_boxes_list[i].float().cpu(), box_idx_token_ids)
            if sel.shape[0] == 0:
                self.invalid += 1
                continue
            if logprobs is not None:
                conf = grounded_scores(sequences[i, prompt_len:].cpu(), logprobs[i], pred_boxes_list[i].shape[0], box_idx_token_ids)[0]
            ious = pairwise_iou(cxcywh_to_xyxy(sel), cxcywh_to_xyxy(gt_boxes_list[i].float().cpu())).max(dim=-1).values
            self.m_iou += float(ious[0])
            if logprobs is not None:
                self.scores.append((conf, float(ious[0])))
            self.hits += 1.0 if float(ious[0]) > self.threshold else 0.0

    def summary(self, device=None):
        t = torch.tensor([self.hits, self.m_iou, self.invalid, self.count], dtype=torch.float64)
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            if device is not None:
                t = t.to(device)
            dist.all_reduce(t)
            t = t.cpu()
        hits, miou, invalid, n = t.tolist()
        n = max(n, 1.0)
        return {f"iou@{self.threshold} accu": hits / n, "m_iou": miou / n, "missing percentage": invalid / n, "count": int(n)}


def lvis_results(sequences, prompt_len, pred_boxes_list, img_ids, labels, img_shapes, box_idx_token_ids, label2cat=None, logprobs=None):
    """eval_lvis.py:147-166: every grounded box as an LVIS detection dict, xywh scaled to (h, w) of the image.  "score" is the
    reference's constant 1.0 (eval_lvis.py:166), or -- with logprobs [bs, new] (GenerateOutput.logprobs) -- exp(log-probability) of the
    region token that selected the box (grounded_scores).  Under generate(grounded=True) (grammar.py) no `<r_k>` is dropped (every k
    is below the image's box count) and that probability is over the image's own boxes."""
    out = []
    for i in range(sequences.shape[0]):
        sel = grounded_boxes(sequences[i, prompt_len:].cpu(), pred_boxes_list[i].float().cpu(), box_idx_token_ids)
        if sel.shape[0] == 0:
            continue
        h, w = img_shapes[i]
        xywh = torch.stack([(sel[:, 0] - 0.5 * sel[:, 2]) * w, (sel[:, 1] - 0.5 * sel[:, 3]) * h, sel[:, 2] * w, sel[:, 3] * h], -1)
        cat = label2cat[labels[i]] if label2cat is not None else labels[i]
        conf = [1.0] * sel.shape[0] if logprobs is None else \
            grounded_scores(sequences[i, prompt_len:].cpu(), logprobs[i], pred_boxes_list[i].shape[0], box_idx_token_ids)
        out += [{"image_id": img_ids[i], "category_id": cat, "bbox": b, "score": c} for b, c in zip(xywh.tolist(), conf)]
    return out
