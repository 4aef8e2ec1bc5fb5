"""rtx_premask_stats (include/rtx.h): what tells whether RTX_OPT_SHADOW_PREMASK took effect lives in a
struct of its own, so rtx_stats, rtx_point_stats and rtx_dark_stats keep the sizes callers were built
against; the ctypes mirror matches the header as gcc lays it out."""
import ctypes
import os
import shutil
import subprocess

import pytest

import rtxpy
from rtxpy import abi


def test_premask_stats_layout_matches_compiled_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rtx_premask_stats));', 'printf("option %d\\n", (int)RTX_OPT_SHADOW_PREMASK);',
             'printf("stats %zu %zu %zu\\n", sizeof(rtx_stats), sizeof(rtx_point_stats), sizeof(rtx_dark_stats));']
    for f, _ in abi.PremaskStats._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rtx_premask_stats, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(rtxpy.REPO_ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(abi.PremaskStats) == 8
    assert int(got["option"]) == abi.RTX_OPT_SHADOW_PREMASK == 16
    assert [int(v) for v in got["stats"].split()] == [ctypes.sizeof(abi.Stats), 24, 16]
    for f, _ in abi.PremaskStats._fields_:
        assert int(got[f]) == getattr(abi.PremaskStats, f).offset, f


def test_premask_stats_leave_the_other_structs_alone():
    other = abi.Stats._fields_ + abi.PointStats._fields_ + abi.DarkStats._fields_
    assert not set(f for f, _ in abi.PremaskStats._fields_) & set(f for f, _ in other)


def test_premask_stats_accessors_reject_null():
    lib = rtxpy.rtx_lib()
    m = abi.PremaskStats()
    assert lib.rtx_get_premask_stats(None, ctypes.byref(m)) == abi.RTX_ERR_ARG
    assert lib.rtx_group_get_premask_stats(None, ctypes.byref(m)) == abi.RTX_ERR_ARG
    assert lib.rtx_group_device_premask_stats(None, 0, ctypes.byref(m)) == abi.RTX_ERR_ARG
