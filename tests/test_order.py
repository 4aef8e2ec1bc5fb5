"""The bucket of k_shadow's sample order (RTX_OPT_SHADOW_ORDER) and the order's definition, on the CPU:
the numpy restatement test_gpu_order.py holds the device to, and the new ABI pieces."""
import ctypes

import numpy as np
import pytest

import order_model as M
import rtxpy
from rtxpy import abi

f32 = np.float32


def test_bucket_edges():
    x = np.array([-2.0, -1.0, np.nextafter(f32(-0.875), f32(-1)), -0.875, -1e-30, -0.0, 0.0, 0.124, 0.125, 0.9999, 1.0, 3.0,
                  np.inf, -np.inf, np.nan], f32)
    # -1e-30 + 1 rounds to 1 in float32, on the device as here: bucket 8
    want = [0, 0, 0, 1, 8, 8, 8, 8, 9, 15, 15, 15, 15, 0, 0]
    assert M.bucket(x).tolist() == want


def test_bucket_is_monotonic_and_covers_the_disc():
    x = np.sort(np.random.default_rng(5).uniform(-1.2, 1.2, 20000).astype(f32))
    b = M.bucket(x)
    assert (np.diff(b) >= 0).all()
    assert set(b.tolist()) == set(range(M.BUCKETS))
    inside = np.abs(x) < 1
    # a bucket is an eighth of the radius wide
    assert np.array_equal(b[inside], np.floor((x[inside].astype(np.float64) + 1) * 8).astype(np.int64))


def test_check_order_accepts_the_stable_sort_only():
    rng = np.random.default_rng(9)
    nl = 300
    buckets = rng.integers(0, M.BUCKETS + 1, M.CAP)  # BUCKETS: a dark sample
    buckets[nl:] = M.BUCKETS
    placed = np.flatnonzero(buckets[:nl] < M.BUCKETS)
    order = placed[np.argsort(buckets[placed], kind="stable")]
    M.check_order(order, buckets, nl)
    swapped = order.copy()
    i = int(np.flatnonzero(np.diff(buckets[order]) == 0)[0])
    swapped[[i, i + 1]] = swapped[[i + 1, i]]  # two of one bucket out of index order
    with pytest.raises(AssertionError):
        M.check_order(swapped, buckets, nl)
    with pytest.raises(AssertionError):
        M.check_order(order[:-1], buckets, nl)
    with pytest.raises(AssertionError):
        M.check_order(placed, buckets, nl)  # index order: buckets not sorted


def test_order_stats_layout_matches_compiled_header(tmp_path):
    import os
    import subprocess
    root = rtxpy.REPO_ROOT
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', '#include "rtx_kat.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(rtx_order_stats));', 'printf("option %d\\n", (int)RTX_OPT_SHADOW_ORDER);',
             'printf("kat %d\\n", (int)RTX_KAT_ORDER);', 'printf("kat_in %d\\n", rtx_kat_in_width[RTX_KAT_ORDER]);',
             'printf("kat_out %d\\n", rtx_kat_out_width[RTX_KAT_ORDER]);', 'printf("kinds %d\\n", (int)RTX_KAT_NKINDS);']
    for f, _ in abi.OrderStats._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rtx_order_stats, {f}));')
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(abi.OrderStats) == 16
    assert int(got["option"]) == abi.RTX_OPT_SHADOW_ORDER == 17
    assert int(got["kat"]) == abi.KAT_ORDER and int(got["kinds"]) == len(abi.KAT_NAMES) == len(abi.KAT_IN) == len(abi.KAT_OUT)
    assert int(got["kat_in"]) == abi.KAT_IN[abi.KAT_ORDER] and int(got["kat_out"]) == abi.KAT_OUT[abi.KAT_ORDER]
    for f, _ in abi.OrderStats._fields_:
        assert int(got[f]) == getattr(abi.OrderStats, f).offset, f


def test_order_stats_accessors_reject_null():
    lib = rtxpy.rtx_lib()
    o = abi.OrderStats()
    assert lib.rtx_get_order_stats(None, ctypes.byref(o)) == abi.RTX_ERR_ARG
    assert lib.rtx_group_get_order_stats(None, ctypes.byref(o)) == abi.RTX_ERR_ARG
    assert lib.rtx_group_device_order_stats(None, 0, ctypes.byref(o)) == abi.RTX_ERR_ARG
    assert not set(f for f, _ in abi.OrderStats._fields_) & set(f for f, _ in abi.Stats._fields_ + abi.PointStats._fields_ + abi.DarkStats._fields_)
