"""bench.py --dump-outputs: dump_arrays turns what one step handed its caller into host arrays -- float32 / float64 only, a fixed
logits sample (the same positions in every run, so two builds compare output for output), and at most 64 MB whatever the batch.
CPU only: the arrays are built from host tensors of the benchmark's shapes."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, L = 32114, 582   # Groma-7B vocabulary (32000 + the box / region tokens) and sequence length at 100 regions


def _bench():
    spec = importlib.util.spec_from_file_location("bench_dump_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _held(images, chunk, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = [torch.randn((min(chunk, images - lo), L, V), generator=g, dtype=torch.float32) for lo in range(0, images, chunk)]
    boxes = [torch.rand((100 - (i % 3), 4), generator=g) for i in range(images)]
    return {"logits": logits, "pred_boxes": boxes, "rows": torch.randn((images, 100 + 401), generator=g)}


def test_dump_arrays_is_float_bounded_and_samples_fixed_positions():
    bench = _bench()
    held = _held(3, 2)
    a, b = bench.dump_arrays(held), bench.dump_arrays(_held(3, 2))
    assert set(a) == {"rows", "pred_boxes", "n_regions", "logits_last", "logits_sample", "logits_sample_index"}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    full = torch.cat(held["logits"]).reshape(3, -1).numpy()
    idx = a["logits_sample_index"].astype(np.int64)
    assert np.array_equal(a["logits_sample"], full[:, idx]) and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["logits_last"], torch.cat(held["logits"])[:, -1].numpy())
    assert a["n_regions"].tolist() == [100, 99, 98] and a["pred_boxes"].shape == (3, 100, 4)
    assert np.array_equal(a["pred_boxes"][1, :99], held["pred_boxes"][1].numpy()) and not a["pred_boxes"][1, 99:].any()


def test_dump_arrays_stays_under_64_mb_at_large_batches():
    bench = _bench()
    images = 160   # more images than logits_last keeps; one [L, V] block is shared by all, so its size is a view
    one = torch.zeros((1, L, V))
    held = {"logits": [one.expand(images, L, V)], "pred_boxes": [torch.zeros((100, 4))] * images,
            "rows": torch.zeros((images, 501))}
    a = bench.dump_arrays(held)
    assert a["logits_last"].shape == (bench.DUMP_LAST_ROWS, V) and a["logits_sample"].shape[0] == images
    assert sum(x.nbytes for x in a.values()) <= 64 << 20


def test_dump_arrays_generate_keeps_exact_token_ids():
    bench = _bench()
    seq = torch.tensor([[1, 32113, 16777217]], dtype=torch.int64)   # 2^24 + 1: not exact in float32
    a = bench.dump_arrays({"sequences": [seq], "pred_boxes": [torch.zeros((100, 4))], "rows": torch.zeros((1, 501))})
    assert a["sequences"].dtype == np.float64 and a["sequences"].tolist() == [[1, 32113, 16777217]]
    assert "logits_sample" not in a
