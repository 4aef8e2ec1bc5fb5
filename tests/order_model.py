"""numpy restatements for k_shadow's sample order (rtx_shadow.hip order_begin): the key's bucket and
what a valid order is.  Shared by test_order.py (CPU) and test_gpu_order.py."""
import numpy as np

BUCKETS = 16  # rtx_device.h RTX_ORD_BUCKETS
CAP = 1024    # RTX_ORD_CAP
f32 = np.float32


def bucket(x):
    """order_bucket in float32: floor((x + 1) * 8) held to 0..15, a NaN in bucket 0"""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        v = np.floor((x + f32(1)) * f32(0.5 * BUCKETS))
    v = np.where(np.isnan(v), f32(0), v)
    return np.clip(v, 0, BUCKETS - 1).astype(np.int64)


def check_order(order, buckets, nl):
    """order: the positions' sample indices; buckets: every sample's bucket (BUCKETS: no place).
    A permutation of the samples with a bucket, buckets non-decreasing along it, indices increasing
    inside a bucket (the counting sort is stable)."""
    order = np.asarray(order, np.int64)
    buckets = np.asarray(buckets, np.int64)
    placed = np.flatnonzero(buckets[:nl] < BUCKETS)
    assert len(order) == len(placed), (len(order), len(placed))
    assert np.array_equal(np.sort(order), placed)
    b = buckets[order]
    assert (np.diff(b) >= 0).all()
    same = np.diff(b) == 0
    assert (np.diff(order)[same] > 0).all()
    # which is the stable sort of the placed indices by bucket
    assert np.array_equal(order, placed[np.argsort(buckets[placed], kind="stable")])
