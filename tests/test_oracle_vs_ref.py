"""Oracle restatement (oracle/roi_nms.c) against the reference's OWN CPU ops (mmcv nms / roi_align, compiled from the reference's
sources into oracle/_ref/libmmcv_ref.so by oracle/build_ref.py).  Their outputs on exactly these inputs are stored in
tests/golden/ref_cpu_ops.npz (generator: tests/golden/make_ref_ops_golden.py), so the comparison runs everywhere; where the
library is built, the live reference is used and must still reproduce the stored vectors."""
import os

import numpy as np
import pytest

from oracle import cref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_cpu_ops.npz")
NMS_SEEDS, NMS_THRS = range(4), (0.3, 0.6)
ROI_SCALES = (1 / 7.0, 1 / 14.0)


def nms_case(seed):
    rng = np.random.default_rng(seed)
    n = 300
    xy = rng.random((n, 2)).astype(np.float32)
    boxes = np.concatenate([xy, xy + 0.03 + 0.25 * rng.random((n, 2)).astype(np.float32)], 1)
    scores = rng.permutation(n).astype(np.float32) / n  # tie-free: the reference's sort is unstable
    return boxes, scores


def roi_case():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 5, 32, 32)).astype(np.float32)
    R = 30
    x1y1 = rng.random((R, 2)).astype(np.float32) * 300
    wh = rng.random((R, 2)).astype(np.float32) * 200 + 5
    rois = np.concatenate([(np.arange(R) % 2)[:, None].astype(np.float32), x1y1, x1y1 + wh], 1)
    return x, rois


def groma_roi_case():
    """a (cx, cy, w, h)*448 ROI as Groma passes it -- x2 < x1 for the reference's CPU op"""
    return np.arange(64, dtype=np.float32).reshape(1, 1, 8, 8), np.array([[0, 5.0, 5.0, 1.0, 1.0]], dtype=np.float32)


def reference_outputs():
    """what the reference's CPU ops return on the cases above (the live library: needs oracle/_ref)"""
    out = {}
    for seed in NMS_SEEDS:
        boxes, scores = nms_case(seed)
        for thr in NMS_THRS:
            out[f"nms_keep_s{seed}_t{thr}"] = cref.ref_nms(boxes, scores, thr)
    x, rois = roi_case()
    for i, scale in enumerate(ROI_SCALES):
        out[f"roi_out_{i}"] = cref.ref_roi_align_avg(x, rois, (14, 14), scale, 2, True)
    x, rois = groma_roi_case()
    out["groma_roi_rejected"] = np.array(cref.ref_roi_align_avg(x, rois, (2, 2), 1.0, 2, True) is None)
    return out


@pytest.fixture(scope="module")
def ref():
    stored = dict(np.load(GOLDEN))
    if cref.ref_available():
        live = reference_outputs()
        assert sorted(live) == sorted(stored)
        for k, v in live.items():
            assert v is not None and np.array_equal(v, stored[k]), k
    return stored


@pytest.mark.parametrize("seed", NMS_SEEDS)
def test_nms_equals_reference_cpu(ref, seed):
    boxes, scores = nms_case(seed)
    for thr in NMS_THRS:
        assert np.array_equal(cref.nms(boxes, scores, thr), ref[f"nms_keep_s{seed}_t{thr}"])


def test_roi_align_equals_reference_cpu_on_legal_rois(ref):
    x, rois = roi_case()
    for i, scale in enumerate(ROI_SCALES):
        got = cref.roi_align_avg(x, rois, (14, 14), scale, 2, True)
        # the CPU implementation pre-computes weights in a different association order: fp32-roundoff agreement
        assert np.allclose(got, ref[f"roi_out_{i}"], rtol=1e-5, atol=1e-6)


def test_reference_cpu_rejects_groma_rois_but_oracle_follows_cuda(ref):
    """the reference CPU op asserts on (cx,cy,w,h)*448 ROIs; the CUDA arithmetic (our oracle) does not."""
    x, rois = groma_roi_case()
    assert bool(ref["groma_roi_rejected"])
    assert np.isfinite(cref.roi_align_avg(x, rois, (2, 2), 1.0, 2, True)).all()
