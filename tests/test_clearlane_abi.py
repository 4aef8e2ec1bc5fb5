"""RTX_OPT_SHADOW_CLEARLANE and rtx_clearlane_stats (include/rtx.h): the option's number and the struct's
layout in the ctypes mirror match the header as gcc reads it, the struct is one of its own (rtx_stats and
the other statistics keep their sizes), and the accessors and the option refuse a null context.  The
option's values (0 and 1 only, default 1) need a context: tests/test_gpu_clearlane.py."""
import ctypes
import os
import shutil
import subprocess

import pytest

import rtxpy
from rtxpy import abi


def test_clearlane_layout_matches_compiled_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rtx_clearlane_stats));', 'printf("option %d\\n", (int)RTX_OPT_SHADOW_CLEARLANE);',
             'printf("stats %zu %zu %zu %zu %zu\\n", sizeof(rtx_stats), sizeof(rtx_point_stats), sizeof(rtx_dark_stats), '
             'sizeof(rtx_order_stats), sizeof(rtx_premask_stats));']
    for f, _ in abi.ClearlaneStats._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rtx_clearlane_stats, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(rtxpy.REPO_ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(abi.ClearlaneStats) == 16
    assert int(got["option"]) == abi.RTX_OPT_SHADOW_CLEARLANE == 20
    assert [int(v) for v in got["stats"].split()] == [ctypes.sizeof(abi.Stats), 24, 16, 16, 8]
    for f, _ in abi.ClearlaneStats._fields_:
        assert int(got[f]) == getattr(abi.ClearlaneStats, f).offset, f


def test_clearlane_stats_leave_the_other_structs_alone():
    other = abi.Stats._fields_ + abi.PointStats._fields_ + abi.DarkStats._fields_ + abi.OrderStats._fields_ + abi.PremaskStats._fields_
    assert not set(f for f, _ in abi.ClearlaneStats._fields_) & set(f for f, _ in other)
    assert [f for f, _ in abi.ClearlaneStats._fields_] == ["clear_points", "clear_rays"]


def test_clearlane_symbols_are_declared_and_exported():
    lib = rtxpy.rtx_lib()
    for name in ("rtx_get_clearlane_stats", "rtx_group_get_clearlane_stats", "rtx_group_device_clearlane_stats"):
        assert name in abi.RTX_SYMBOLS
        assert getattr(lib, name) is not None


def test_clearlane_accessors_and_option_reject_null():
    lib = rtxpy.rtx_lib()
    m = abi.ClearlaneStats()
    assert lib.rtx_get_clearlane_stats(None, ctypes.byref(m)) == abi.RTX_ERR_ARG
    assert lib.rtx_group_get_clearlane_stats(None, ctypes.byref(m)) == abi.RTX_ERR_ARG
    assert lib.rtx_group_device_clearlane_stats(None, 0, ctypes.byref(m)) == abi.RTX_ERR_ARG
    assert lib.rtx_set_option(None, abi.RTX_OPT_SHADOW_CLEARLANE, 1) == abi.RTX_ERR_ARG
    assert lib.rtx_group_set_option(None, abi.RTX_OPT_SHADOW_CLEARLANE, 1) == abi.RTX_ERR_ARG
