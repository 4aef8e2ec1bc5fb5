"""Tile-list renders' and adaptive passes' C-ABI (rtx_render_tiles*, rtx_render_adaptive*, include/rtx.h) on a
CPU-only host: declarations, exports, the stats struct's layout, null contexts, and the engine's --adaptive flag."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import conftest as C
import rtxpy
from rtxpy import abi

HEADER = os.path.join(rtxpy.REPO_ROOT, "include", "rtx.h")
INT_FUNCS = ["rtx_render_tiles", "rtx_render_tiles_device", "rtx_render_adaptive", "rtx_render_adaptive_device",
             "rtx_get_adaptive_stats"]


def test_header_declares_and_library_exports_the_new_functions():
    text = open(HEADER).read()
    lib = ctypes.CDLL(rtxpy.LIBRTX)
    for f in INT_FUNCS:
        assert re.search(r"^\s*int\s+%s\(" % f, text, re.M), f
        assert f in abi.RTX_SYMBOLS and hasattr(lib, f), f
    # the launchers and loaders behind them stay out of the exported symbols
    for f in ("rtx_launch_tile_fold", "rtx_launch_tile_select", "rtx_launch_tile_out", "rtx_launch_tiles_check", "rtx_load_adaptive"):
        assert not hasattr(lib, f), f


def test_adaptive_stats_layout_matches_compiled_header(tmp_path):
    """every field offset and the size of abi.AdaptiveStats against rtx.h as gcc lays it out; the structs the existing
    entry points take keep their sizes"""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rtx_adaptive_stats));',
             'printf("pass_params %zu\\n", sizeof(rtx_pass_params));', 'printf("pass_stats %zu\\n", sizeof(rtx_pass_stats));']
    for f, _ in abi.AdaptiveStats._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rtx_adaptive_stats, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(abi.AdaptiveStats) == 56
    assert int(got["pass_params"]) == ctypes.sizeof(abi.PassParams) and int(got["pass_stats"]) == ctypes.sizeof(abi.PassStats)
    for f, _ in abi.AdaptiveStats._fields_:
        assert int(got[f]) == getattr(abi.AdaptiveStats, f).offset, f


def test_null_contexts_fail_cleanly():
    lib = rtxpy.rtx_lib()
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scene1.json"), base_dir=C.GOLDEN)
    frame = scene.frame(16, 16)
    scene.close()
    p, pp, st = rtxpy.default_params(), rtxpy.pass_params(passes=2, target_error=0.1), abi.AdaptiveStats()
    tiles = (ctypes.c_uint32 * 1)(0)
    f, q = ctypes.byref(frame), ctypes.byref(p)
    assert lib.rtx_render_tiles(None, f, q, tiles, 1, None, None) == abi.RTX_ERR_ARG
    assert b"null" in lib.rtx_last_error()
    assert lib.rtx_render_tiles_device(None, f, q, None, 0, None, None, None) == abi.RTX_ERR_ARG
    assert lib.rtx_render_adaptive(None, f, q, ctypes.byref(pp), None, None, None, None) == abi.RTX_ERR_ARG
    assert lib.rtx_render_adaptive_device(None, f, q, ctypes.byref(pp), None, None, None, None, None) == abi.RTX_ERR_ARG
    assert lib.rtx_get_adaptive_stats(None, ctypes.byref(st)) == abi.RTX_ERR_ARG


def run(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, timeout=120, **kw)


def test_engine_help_names_adaptive():
    p = run([rtxpy.ENGINE, "--help"])
    assert p.returncode == 0 and "--adaptive" in p.stdout


@pytest.mark.parametrize("flags,word", [(["--adaptive"], "--target-error"), (["--adaptive", "--passes", "8", "--aa"], "--target-error"),
                                        (["--adaptive", "--target-error", "0"], "--target-error"),
                                        (["--adaptive", "--target-error", "0.01", "--gpus", "2"], "one GPU")])
def test_engine_refuses_adaptive_before_any_device(tmp_path, flags, word):
    """without a target error (a usage error), and on several GPUs like the other pass flags"""
    out = tmp_path / "o.tif"
    p = run([rtxpy.ENGINE, os.path.join(C.SCENES, "scene1.json"), str(out), "16", "16"] + flags)
    assert p.returncode == 1, p.stdout + p.stderr
    assert word in p.stdout and "Loading scene" not in p.stdout and "Commencing" not in p.stdout
    assert not out.exists()
