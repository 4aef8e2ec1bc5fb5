"""Multi-pass and adaptive rendering on device groups (rtx_group_render_passes, rtx_group_render_adaptive,
include/rtx.h) on a CPU-only host: declarations, exports, the exchange statistics' layout, null groups, and the host
reference of the pass records the final gather moves (rtx_pass_pack_host / rtx_pass_unpack_host)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import conftest as C
import rtxpy
from rtxpy import abi

HEADER = os.path.join(rtxpy.REPO_ROOT, "include", "rtx.h")
INT_FUNCS = ["rtx_group_render_passes", "rtx_group_get_pass_stats", "rtx_group_render_adaptive", "rtx_group_get_adaptive_stats",
             "rtx_group_get_exchange_stats", "rtx_pass_pack_host", "rtx_pass_unpack_host", "rtx_pass_pack_device",
             "rtx_pass_unpack_device"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_header_declares_and_library_exports_the_new_functions():
    text = open(HEADER).read()
    lib = ctypes.CDLL(rtxpy.LIBRTX)
    for f in INT_FUNCS:
        assert re.search(r"^\s*int\s+%s\(" % f, text, re.M), f
        assert f in abi.RTX_SYMBOLS and hasattr(lib, f), f
    # the launchers behind them and the shared argument check stay out of the exported symbols
    for f in ("rtx_launch_stat_pack", "rtx_launch_stat_scatter", "rtx_launch_list_shard", "rtx_launch_pass_pack",
              "rtx_launch_pass_unpack", "rtx_passes_args_check"):
        assert not hasattr(lib, f), f
    assert "have no such entry" not in text


def test_exchange_stats_layout_matches_compiled_header(tmp_path):
    """every field offset and the size of abi.GroupExchangeStats against rtx.h as gcc lays it out; the structs the
    group entries reuse keep their sizes"""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rtx_group_exchange_stats));',
             'printf("pass_stats %zu\\n", sizeof(rtx_pass_stats));', 'printf("adaptive_stats %zu\\n", sizeof(rtx_adaptive_stats));']
    for f, _ in abi.GroupExchangeStats._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rtx_group_exchange_stats, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(abi.GroupExchangeStats) == 32
    assert int(got["pass_stats"]) == ctypes.sizeof(abi.PassStats) and int(got["adaptive_stats"]) == ctypes.sizeof(abi.AdaptiveStats)
    for f, _ in abi.GroupExchangeStats._fields_:
        assert int(got[f]) == getattr(abi.GroupExchangeStats, f).offset, f


def test_null_groups_fail_cleanly():
    lib = rtxpy.rtx_lib()
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scene1.json"), base_dir=C.GOLDEN)
    frame = scene.frame(16, 16)
    scene.close()
    p, pp = rtxpy.default_params(), rtxpy.pass_params(passes=2, target_error=0.1)
    f, q, o = ctypes.byref(frame), ctypes.byref(p), ctypes.byref(pp)
    assert lib.rtx_group_render_passes(None, f, q, o, None, None, None) == abi.RTX_ERR_ARG
    assert b"null" in lib.rtx_last_error()
    assert lib.rtx_group_render_adaptive(None, f, q, o, None, None, None, None) == abi.RTX_ERR_ARG
    assert lib.rtx_group_get_pass_stats(None, ctypes.byref(abi.PassStats())) == abi.RTX_ERR_ARG
    assert lib.rtx_group_get_adaptive_stats(None, ctypes.byref(abi.AdaptiveStats())) == abi.RTX_ERR_ARG
    assert lib.rtx_group_get_exchange_stats(None, ctypes.byref(abi.GroupExchangeStats())) == abi.RTX_ERR_ARG
    assert lib.rtx_pass_pack_device(None, None, None, None, 8, 8, 0, 1, None, None) == abi.RTX_ERR_ARG
    assert lib.rtx_pass_unpack_device(None, None, 8, 8, 0, 1, None, None, None, None) == abi.RTX_ERR_ARG


W, H, SHARDS = 20, 61, 5  # 3 x 8 = 24 tiles, cut by both edges, over 5 shards


def frame_arrays():
    """three arrays of distinct bit patterns, NaNs with payloads, infinities and -0.0 among them"""
    rng = np.random.default_rng(7)
    rgb = rng.integers(0, 2 ** 32, (H, W, 3), dtype=np.uint64).astype(np.uint32)
    z = rng.integers(0, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32)
    var = rng.integers(0, 2 ** 32, (H, W, 3), dtype=np.uint64).astype(np.uint32)
    rgb[0, 0] = (0x7FC00001, 0xFFC12345, 0x7F800001)  # quiet NaNs with payloads, a signalling one
    rgb[60, 19] = (0x80000000, 0x7F800000, 0xFF800000)  # -0.0, +inf, -inf: the frame's last pixel
    z[7, 7], z[8, 8] = 0x80000000, 0x7FA00000
    var[33, 16] = (0xFFFFFFFF, 0x80000000, 0x00000001)
    return rgb.view(np.float32), z.view(np.float32), var.view(np.float32)


def test_pass_records_hold_every_pixel_once_bit_for_bit():
    rgb, z, var = frame_arrays()
    tiles_x, tiles = 3, 24
    seen = np.zeros((H, W), np.int32)
    total = 0
    for off in range(SHARDS):
        rec = rtxpy.pass_pack(rgb, z, var, off, SHARDS)
        n_tiles = len(range(off, tiles, SHARDS))
        assert rec.shape == (64 * n_tiles, 8) == (rtxpy.rtx_lib().rtx_tile_pack_count(W, H, off, SHARDS), 8)
        total += n_tiles
        r = bits(rec)
        for i in range(rec.shape[0]):
            t, p = off + (i >> 6) * SHARDS, i & 63
            x, y = (t % tiles_x) * 8 + (p & 7), (t // tiles_x) * 8 + (p >> 3)
            if x < W and y < H:
                seen[y, x] += 1
                assert np.array_equal(r[i, 0:3], bits(rgb)[y, x]) and r[i, 3] == bits(z)[y, x]
                assert np.array_equal(r[i, 4:7], bits(var)[y, x]) and r[i, 7] == 0
            else:
                assert not r[i].any()  # a lane outside the frame packs as zeros
    assert total == tiles and np.all(seen == 1)


def test_unpacking_every_shard_rebuilds_the_frame_and_null_outputs_are_skipped():
    rgb, z, var = frame_arrays()
    recs = [rtxpy.pass_pack(rgb, z, var, off, SHARDS) for off in range(SHARDS)]
    poison = 0x7FE5C3E1
    out = [np.full(a.shape, poison, np.uint32).view(np.float32) for a in (rgb, z, var)]
    for off, rec in enumerate(recs):
        rtxpy.pass_unpack(rec, (H, W), off, SHARDS, *out)
    for got, want in zip(out, (rgb, z, var)):
        assert np.array_equal(bits(got), bits(want))
    # one shard alone touches its own pixels only
    one = [np.full(a.shape, poison, np.uint32).view(np.float32) for a in (rgb, z, var)]
    rtxpy.pass_unpack(recs[2], (H, W), 2, SHARDS, *one)
    tile_of = np.kron(np.arange(24).reshape(8, 3), np.ones((8, 8), np.int64))[:H, :W]
    own = tile_of % SHARDS == 2
    assert np.array_equal(bits(one[1])[own], bits(z)[own]) and np.all(bits(one[1])[~own] == poison)
    assert np.array_equal(bits(one[0])[own], bits(rgb)[own]) and np.all(bits(one[0])[~own] == poison)
    # each output alone, the others NULL
    for keep in range(3):
        only = [np.full(a.shape, poison, np.uint32).view(np.float32) if i == keep else None for i, a in enumerate((rgb, z, var))]
        for off, rec in enumerate(recs):
            rtxpy.pass_unpack(rec, (H, W), off, SHARDS, *only)
        assert np.array_equal(bits(only[keep]), bits((rgb, z, var)[keep]))
    lib = rtxpy.rtx_lib()
    assert lib.rtx_pass_unpack_host(recs[0].ctypes.data, W, H, 0, SHARDS, None, None, None) == abi.RTX_OK
    assert lib.rtx_pass_unpack_host(None, W, H, 0, SHARDS, None, None, None) == abi.RTX_ERR_ARG
    assert lib.rtx_pass_unpack_host(recs[0].ctypes.data, W, H, 5, SHARDS, None, None, None) == abi.RTX_ERR_ARG
    assert lib.rtx_pass_pack_host(rgb.ctypes.data, z.ctypes.data, None, W, H, 0, SHARDS, recs[0].ctypes.data) == abi.RTX_ERR_ARG
