"""RTX_OPT_SHADOW_SPEC and RTX_KAT_SPEC0 (include/rtx.h, include/rtx_kat.h): the Python mirror matches
the headers as gcc reads them, and the option takes 0 and 1 only."""
import os
import shutil
import subprocess

import pytest

import rtxpy
from rtxpy import abi


def test_spec_option_and_kat_match_compiled_headers(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include "rtx.h"', '#include "rtx_kat.h"', "int main(void) {",
             'printf("option %d\\n", (int)RTX_OPT_SHADOW_SPEC);', 'printf("kat %d\\n", (int)RTX_KAT_SPEC0);',
             'printf("kat_in %d\\n", rtx_kat_in_width[RTX_KAT_SPEC0]);', 'printf("kat_out %d\\n", rtx_kat_out_width[RTX_KAT_SPEC0]);',
             'printf("dark_in %d\\n", rtx_kat_in_width[RTX_KAT_DARK]);', 'printf("dark_out %d\\n", rtx_kat_out_width[RTX_KAT_DARK]);',
             'printf("kinds %d\\n", (int)RTX_KAT_NKINDS);', "return 0; }"]
    src = tmp_path / "spec.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "spec"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(rtxpy.REPO_ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {k: int(v) for k, v in (l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert got["option"] == abi.RTX_OPT_SHADOW_SPEC == 18
    assert got["kat"] == abi.KAT_SPEC0 == 21
    assert got["kinds"] == len(abi.KAT_NAMES) == len(abi.KAT_IN) == len(abi.KAT_OUT)
    # the new kind reads RTX_KAT_DARK's record and writes its layout
    assert got["kat_in"] == got["dark_in"] == abi.KAT_IN[abi.KAT_SPEC0] == abi.KAT_IN[abi.KAT_DARK]
    assert got["kat_out"] == got["dark_out"] == abi.KAT_OUT[abi.KAT_SPEC0] == abi.KAT_OUT[abi.KAT_DARK]
    assert abi.KAT_NAMES[abi.KAT_SPEC0] == "spec0"


def test_spec_option_rejects_a_null_context():
    assert rtxpy.rtx_lib().rtx_set_option(None, abi.RTX_OPT_SHADOW_SPEC, 1) == abi.RTX_ERR_ARG
