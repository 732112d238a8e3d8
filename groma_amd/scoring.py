"""Host side of GromaModel.score(): which rows of the expanded sequence get a head launch, and what each is scored against.

Pure host code on CPU tensors (no device value enters or leaves), so it is tested without a GPU (tests/test_score_host.py).
The semantics are those of forward(labels=...) (R: groma/model/groma.py:404-415, HF's shift): the logits of expanded position p
score the label at p + 1, the first label of a row is never scored, IGNORE_INDEX labels are skipped."""
from types import SimpleNamespace

import torch

from .constants import IGNORE_INDEX

I32, I64 = torch.int32, torch.int64


def score_plan(labels, positions, vocab_size, ignore_index=IGNORE_INDEX):
    """labels int64 [bs, L]: the spliced (expanded) labels; positions int64 [bs, L]: for every expanded position the index of the
    caller's label that sits there (any value where labels == ignore_index).  Returns a namespace of host tensors, one entry per
    scored label in (batch row, position) order:
      rows      int32  flat row b * L + p - 1 of the [bs * L, T] residual stream whose logits score the label at (b, p), p >= 1
      targets   int64  that label
      owner     int64  b
      positions int64  the caller's own position of that label
      counts    int64 [bs]  scored labels per batch row
    Raises ValueError (before anything is launched) for a scored target outside [0, vocab_size)."""
    labels = torch.as_tensor(labels, dtype=I64)
    positions = torch.as_tensor(positions, dtype=I64)
    if labels.dim() != 2 or labels.shape != positions.shape:
        raise ValueError("labels and positions must be two [bs, L] tensors of one shape")
    bs, L = labels.shape
    keep = labels != ignore_index
    keep[:, :1] = False  # no position in front of it: HF's shift never scores the first label
    b, p = keep.nonzero(as_tuple=True)  # row-major: batch row ascending, position ascending inside a row
    targets = labels[b, p]
    bad = (targets < 0) | (targets >= vocab_size)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise ValueError(f"label {int(targets[i])} (row {int(b[i])}, caller position {int(positions[b[i], p[i]])}) is outside the "
                         f"vocabulary [0, {vocab_size})")
    return SimpleNamespace(rows=(b * L + p - 1).to(I32), targets=targets.contiguous(), owner=b.contiguous(),
                           positions=positions[b, p].contiguous(), counts=torch.bincount(b, minlength=bs).to(I64))
