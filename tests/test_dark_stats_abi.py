"""rtx_dark_stats (include/rtx.h): the counters of RTX_OPT_SHADOW_DARK live in a struct of their own,
so rtx_stats and rtx_point_stats keep the sizes callers were built against; the ctypes mirror
matches the header as gcc lays it out."""
import ctypes
import os
import shutil
import subprocess

import pytest

import rtxpy
from rtxpy import abi


def test_dark_stats_layout_matches_compiled_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rtx_dark_stats));', 'printf("option %d\\n", (int)RTX_OPT_SHADOW_DARK);']
    for f, _ in abi.DarkStats._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rtx_dark_stats, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(rtxpy.REPO_ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(abi.DarkStats) == 16
    assert int(got["option"]) == abi.RTX_OPT_SHADOW_DARK == 15
    for f, _ in abi.DarkStats._fields_:
        assert int(got[f]) == getattr(abi.DarkStats, f).offset, f


def test_dark_stats_leave_the_other_structs_alone():
    assert ctypes.sizeof(abi.PointStats) == 24
    assert not set(f for f, _ in abi.DarkStats._fields_) & set(f for f, _ in abi.Stats._fields_ + abi.PointStats._fields_)


def test_dark_stats_accessors_reject_null():
    lib = rtxpy.rtx_lib()
    d = abi.DarkStats()
    assert lib.rtx_get_dark_stats(None, ctypes.byref(d)) == abi.RTX_ERR_ARG
    assert lib.rtx_group_get_dark_stats(None, ctypes.byref(d)) == abi.RTX_ERR_ARG
    assert lib.rtx_group_device_dark_stats(None, 0, ctypes.byref(d)) == abi.RTX_ERR_ARG
