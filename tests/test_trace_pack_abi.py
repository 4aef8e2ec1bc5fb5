"""RTX_OPT_TRACE_PACK (include/rtx.h): the Python mirror matches the header as gcc reads it, the option is
on by default in the library's source, and it takes 0, 1 and the four segment sizes only."""
import os
import re
import shutil
import subprocess

import pytest

import rtxpy
from rtxpy import abi

CSRC = os.path.join(rtxpy.REPO_ROOT, "c-raytracer_amd", "csrc")


def test_trace_pack_option_matches_the_compiled_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    src = tmp_path / "pack.c"
    src.write_text('#include <stdio.h>\n#include "rtx.h"\nint main(void) { printf("%d %d\\n", (int)RTX_OPT_TRACE_PACK, '
                   '(int)RTX_OPT_SHADOW_SPEC); return 0; }\n')
    exe = tmp_path / "pack"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(rtxpy.REPO_ROOT, "include"), str(src), "-o", str(exe)], check=True)
    pack, spec = (int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert pack == abi.RTX_OPT_TRACE_PACK == 19
    assert spec == abi.RTX_OPT_SHADOW_SPEC == 18  # the options before it keep their ids


def test_trace_pack_default_and_values_in_the_source():
    with open(os.path.join(CSRC, "rtx_internal.h")) as fh:
        internal = fh.read()
    assert re.search(r"uint32_t\s+opt_trace_pack\s*=\s*1\s*;", internal)  # on by default
    seg = int(re.search(r"#define\s+RTX_TRACE_PACK_SEG\s+(\d+)u", internal).group(1))
    assert seg in (512, 1024, 2048, 4096)
    with open(os.path.join(CSRC, "rtx_ctx.cpp")) as fh:
        ctx = fh.read()
    case = ctx[ctx.index("case RTX_OPT_TRACE_PACK:"):]
    case = case[:case.index("return RTX_OK;")]
    assert sorted(int(v) for v in re.findall(r"value != (\d+)", case)) == [0, 1, 512, 1024, 2048, 4096]


def test_trace_pack_option_rejects_a_null_context():
    assert rtxpy.rtx_lib().rtx_set_option(None, abi.RTX_OPT_TRACE_PACK, 1) == abi.RTX_ERR_ARG
