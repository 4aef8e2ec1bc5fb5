"""One context reused across frame sizes gives what a fresh context gives, byte for byte.

A context keeps grow-only device scratch (rtx_internal.h DevBuf: the framebuffer, the render's work
buffers, the queries' and the denoiser's copies) and sizes shared areas from whichever call comes
first (the k_shadow spill area, the k_trace overflow stack, the query counters).  A capacity that
outlives its buffer, or scratch one call sizes too small for the next, shows here as a different
output or a fault.  Three rounds on one context, 64x48, then 128x96 (every buffer grows), then 32x24
(every buffer is larger than needed); each round runs the host-buffer entry points in turn and
every output must equal the same call's on a context opened for that size alone.

Two scenes: scene3 (a few spheres: the linear shadow walk, no tree) and the dragon stand-in with
RTX_OPT_SHADOW_LDS_STACK 1, so that k_shadow's lane stacks spill to the shared area; there the scene is
uploaded again before every round and the context's very first call is the shadow query, which then
sizes the spill area itself.
"""
import os

import numpy as np
import pytest

import conftest as C
import rays_frames as RF
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (128, 96), (32, 24)]
CALLS = ("render_rgb", "render_z", "post", "hit_t", "hit_object", "hit_n", "shadow_blocked", "shadow_t", "features", "denoise")


def load(name):
    if name == "scene5":
        return RF.load_scene(name)  # the dragon stand-in
    return rtxpy.Scene.load(os.path.join(C.SCENES, name + ".json"), base_dir=C.GOLDEN)


def open_ctx(scene, lds):
    r = rtxpy.Renderer(0)
    if lds:
        r.set_option(abi.RTX_OPT_SHADOW_LDS_STACK, lds)
    r.upload(scene)
    return r


def frame_rays(r, frame):
    import torch
    d = torch.zeros((frame.width * frame.height, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # torch filled it on its stream, the context works on its own
    r.frame_rays_device(frame, d.data_ptr())
    rays = d.cpu().numpy()
    return rays[:, 0:3].copy(), rays[:, 4:7].copy()


def shadow_rays_of(scene, o, d, t):
    """from every hit point towards the first emitter (which never blocks); a miss is an idle lane"""
    light = scene.emitters()[0]
    L = np.array(list(scene.objects()[light].p0), np.float32)
    P = o + t[:, None] * d
    v = L[None, :] - P
    dist = np.linalg.norm(v, axis=1).astype(np.float32)
    ok = (t > 0) & (dist > 0)
    sd = np.where(ok[:, None], v / np.where(ok, dist, 1)[:, None], d).astype(np.float32)
    return P.astype(np.float32), sd, np.where(ok, dist, 0).astype(np.float32), int(light)


def run_round(r, scene, frame, o, d, first_shadow=None):
    """every host-buffer entry point once; first_shadow: shadow rays to trace before anything else"""
    out = {}
    if first_shadow is not None:
        first = r.shadow_rays(*first_shadow[:3], light_object=first_shadow[3])
    rgb, z = r.render(frame, rtxpy.params_from_args(["-g", "path", "-n", "4"], seed=11))
    out["render_rgb"], out["render_z"] = rgb, z
    out["post"] = r.postprocess(rtxpy.post_from_args(["--mist", "2", "20", "lin", "0.5", "0.6", "0.7"]), rgb, z)
    hits = r.trace_rays(o, d)
    out["hit_t"], out["hit_object"], out["hit_n"] = hits["t"], hits["object"], hits["n"]
    so, sd, dist, light = shadow_rays_of(scene, o, d, hits["t"])
    sh = r.shadow_rays(so, sd, dist, light_object=light)
    out["shadow_blocked"], out["shadow_t"] = sh["blocked"], sh["transmittance"]
    if first_shadow is not None:
        assert np.array_equal(first["blocked"], sh["blocked"])
        assert first["transmittance"].tobytes() == sh["transmittance"].tobytes()
    feat = r.features(frame)
    out["features"] = feat
    out["denoise"] = r.denoise(rgb, feat)
    assert set(out) == set(CALLS)
    return out, (so, sd, dist, light)


@pytest.mark.parametrize("name,lds", [("scene3", 0), ("scene5", 1)])
def test_reused_context_equals_fresh_contexts(name, lds):
    scene = load(name)
    reused = None
    try:
        for k, (w, h) in enumerate(SIZES):
            frame = scene.frame(w, h)
            fresh = open_ctx(scene, lds)
            try:
                o, d = frame_rays(fresh, frame)
                ref, ref_shadow = run_round(fresh, scene, frame, o, d)
                st = fresh.stats()
            finally:
                fresh.close()
            if lds:  # the walk over an 8-wide tree deeper than one LDS entry and the root: the spill area is in use
                assert st.shadow_walk == abi.RTX_WALK_W8 and st.wide_depth > lds + 1, (st.shadow_walk, st.wide_depth)
            else:
                assert st.shadow_walk == abi.RTX_WALK_LINEAR
            assert (ref["hit_t"] > 0).any()
            met = ref["shadow_blocked"] | (ref["shadow_t"] != 1).any(axis=1)  # (the stand-in is transparent: it filters)
            assert met.any() and not met.all()
            print(f"{name} {w}x{h}: {int((ref['hit_t'] > 0).sum())} hits, {int(met.sum())} shadow rays blocked or filtered")
            if reused is None:
                reused = open_ctx(scene, lds)
            elif lds:
                reused.upload(scene)
            got, _ = run_round(reused, scene, frame, o, d, first_shadow=ref_shadow if lds and k == 0 else None)
            for call in CALLS:
                a, b = np.ascontiguousarray(got[call]), np.ascontiguousarray(ref[call])
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), (name, (w, h), call)
    finally:
        if reused is not None:
            reused.close()
        scene.close()
