"""rtx_point_stats (include/rtx.h): the counters of RTX_OPT_SHADOW_POINT live beside rtx_stats, whose
size stays what callers were built against; the ctypes mirror matches the header as gcc lays it out."""
import ctypes
import os
import shutil
import subprocess

import pytest

import rtxpy
from rtxpy import abi


def test_point_stats_layout_matches_compiled_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rtx_point_stats));']
    for f, _ in abi.PointStats._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rtx_point_stats, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(rtxpy.REPO_ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(abi.PointStats) == 24
    for f, _ in abi.PointStats._fields_:
        assert int(got[f]) == getattr(abi.PointStats, f).offset, f


def test_point_stats_accessors_reject_null():
    lib = rtxpy.rtx_lib()
    p = abi.PointStats()
    assert lib.rtx_get_point_stats(None, ctypes.byref(p)) == abi.RTX_ERR_ARG
    assert lib.rtx_group_get_point_stats(None, ctypes.byref(p)) == abi.RTX_ERR_ARG
    assert lib.rtx_group_device_point_stats(None, 0, ctypes.byref(p)) == abi.RTX_ERR_ARG
