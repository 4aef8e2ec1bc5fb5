"""bench.py's plain one-GPU run end to end: the timed steps and the line, nothing else, and
`--dump-outputs` writing the frame of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import conftest as C


@pytest.mark.gpu
def test_gpu_plain_bench_line_and_dumped_frame(tmp_path):
    """a plain run (no --full) carries the headline keys, `steps` timed steps and none of the side
    legs; the dumped frame is the one the same scene, flags, seed and RNG render through the
    library (bit for bit: the counter RNG makes the frame a function of its inputs)"""
    import rtxpy
    from rtxpy import abi
    w, h = 100, 60  # neither a multiple of the 8x8 tile
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(C.ROOT, "bench.py"), "--gpus", "1", "--scene", "scene3", "--width", str(w),
           "--height", str(h), "--spp", "2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(dump)]
    p = subprocess.run(cmd, cwd=C.ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "Mrays/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    rays = out["config"]["rays_per_frame"]
    assert abs(out["value"] - rays / out["ms_per_step"] / 1e3) <= 0.01 * out["value"]
    assert out["roofline"] is None and out["cpu_baseline"] is None
    assert not {"rng_strat_frame", "cpu_port", "postprocess", "bvh_build"} & set(out)

    rgb, z = np.load(dump / "rgb.npy"), np.load(dump / "z.npy")
    assert sorted(os.listdir(dump)) == ["rgb.npy", "z.npy"]
    assert rgb.dtype == z.dtype == np.float32 and rgb.shape == (h, w, 3) and z.shape == (h, w)
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scene3.json"), base_dir=C.GOLDEN)
    params = rtxpy.params_from_args(["-g", "path", "-n", "2"], seed=1)
    params.rng = abi.RTX_RNG_COUNTER
    r = rtxpy.Renderer(0)
    try:
        r.upload(scene)
        want_rgb, want_z = r.render(scene.frame(w, h), params)
    finally:
        r.close()
    assert np.array_equal(rgb, np.asarray(want_rgb).reshape(h, w, 3))
    assert np.array_equal(z, np.asarray(want_z).reshape(h, w))
    assert (z > 0).any() and rgb.max() > 0
