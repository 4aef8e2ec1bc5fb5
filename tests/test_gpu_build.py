"""GPU BVH builders (csrc/rtx_build.hip via rtx_set_builder(RTX_BUILD_LBVH_GPU /
RTX_BUILD_PLOC_GPU / RTX_BUILD_SAH_GPU)).

Closest-hit answers do not depend on the tree (up to exact ties), so frames rendered over the
GPU-built LBVH must match the reference goldens exactly as well as frames over the host SAH
tree do, and the z-buffer must equal the SAH render's; shadow transmittance products may be
formed in another order (1-ulp-level colour differences, inside the frame tolerance).
"""
import numpy as np
import pytest

import conftest as C
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

CONFIGS = ["s1_amb", "s3_path2", "s5_path2", "s6_amb", "st_amb"]


@pytest.fixture(scope="module")
def renderer():
    r = rtxpy.Renderer(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def _defaults(renderer):
    yield
    renderer.set_builder(abi.RTX_BUILD_SAH_GPU)
    renderer.set_option(abi.RTX_OPT_SHADOW_WALK, abi.RTX_WALK_AUTO)
    renderer.set_option(abi.RTX_OPT_BVH_LEAF, 1)


def render(r, builder, scene, frame, params):
    r.set_builder(builder)
    r.set_option(abi.RTX_OPT_SHADOW_WALK, abi.RTX_WALK_W8)  # the 8-wide tree on small scenes too
    r.upload(scene)
    rgb, z = r.render(frame, params)
    return rgb, z, r.stats()


GPU_BUILDERS = [abi.RTX_BUILD_LBVH_GPU, abi.RTX_BUILD_PLOC_GPU, abi.RTX_BUILD_SAH_GPU]
IDS = ["lbvh", "ploc", "sahgpu"]


@pytest.mark.parametrize("builder", GPU_BUILDERS, ids=IDS)
@pytest.mark.parametrize("name", CONFIGS)
def test_gpu_builder_frames_match(renderer, name, builder):
    scene, frame, params, m = C.load_config(name)
    a, za, sa = render(renderer, abi.RTX_BUILD_SAH_HOST, scene, frame, params)
    b, zb, sb = render(renderer, builder, scene, frame, params)
    assert sb.builder == builder and sa.builder == abi.RTX_BUILD_SAH_HOST
    assert sb.bvh_depth <= 63 and sb.build_ms > 0
    # the 8-wide shadow tree collapsed on the device from the device-built records
    assert sb.shadow_walk == abi.RTX_WALK_W8 and sb.wide_depth >= 1 and sb.wide_nodes >= 1
    assert np.array_equal(za, zb), name  # closest hits do not depend on the tree
    assert (sa.closest_rays, sa.shadow_rays) == (sb.closest_rays, sb.shadow_rays)
    ref_rgb, ref_z = C.golden_frame(name + "_o2")
    ok, info = C.compare_const(b, zb, ref_rgb, ref_z)
    assert ok, info
    assert np.abs(a - b).max() <= 1e-5 * max(1.0, float(np.abs(a).max())), name


@pytest.mark.parametrize("builder", GPU_BUILDERS, ids=IDS)
def test_gpu_builder_deterministic_and_tiny_scenes(renderer, builder):
    scene, frame, params, _ = C.load_config("s5_path2")
    a, za, st = render(renderer, builder, scene, frame, params)
    b, zb, _ = render(renderer, builder, scene, frame, params)
    assert np.array_equal(a, b) and np.array_equal(za, zb)
    assert st.bvh_nodes == st.bvh_prims - 1  # single-primitive leaves (the default): a full binary tree
    # scene1: 3 spheres + a light -> with leaves of up to 4 primitives, a single-leaf root
    renderer.set_option(abi.RTX_OPT_BVH_LEAF, 4)
    scene, frame, params, _ = C.load_config("s1_amb")
    try:
        a, za, st = render(renderer, builder, scene, frame, params)
    finally:
        renderer.set_option(abi.RTX_OPT_BVH_LEAF, 1)
    assert st.bvh_nodes == 0
    o_rgb, o_z = C.golden_frame("s1_amb_o2")
    ok, info = C.compare_const(a, za, o_rgb, o_z)
    assert ok, info
    with pytest.raises(rtxpy.RtxError):
        renderer.set_builder(7)
    renderer.set_builder(abi.RTX_BUILD_SAH_GPU)


@pytest.mark.parametrize("leaf", [2, 4])
def test_gpu_ploc_multi_primitive_leaves(renderer, leaf):
    """Leaves of up to `leaf` primitives: each subtree of at most that many primitives becomes one
    leaf of a contiguous range (depth-first leaf order); the frame stays exact."""
    scene, frame, params, _ = C.load_config("s3_path2")
    renderer.set_option(abi.RTX_OPT_BVH_LEAF, leaf)
    try:
        b, zb, sb = render(renderer, abi.RTX_BUILD_PLOC_GPU, scene, frame, params)
    finally:
        renderer.set_option(abi.RTX_OPT_BVH_LEAF, 1)
    assert sb.bvh_nodes < sb.bvh_prims - 1
    ref_rgb, ref_z = C.golden_frame("s3_path2_o2")
    ok, info = C.compare_const(b, zb, ref_rgb, ref_z)
    assert ok, info


@pytest.mark.parametrize("name", ["s5_path2", "s6_amb", "s3_path2", "st_amb"])
def test_gpu_sah_device_builds_the_host_tree(renderer, name):
    """RTX_BUILD_SAH_GPU runs bvh_build.cpp's binned SAH on the device (same bins, same float
    costs, same split order, stable partitions on both sides): with single-primitive leaves it
    builds the host's tree node for node, primitive for primitive, so the 8-wide collapse, every
    per-ray traversal count and every pixel are the same as over the host build (the dragon and
    Menger stand-ins included; test_gpu_sah_device_collapse_equals_host_collapse compares the
    8-wide trees entry by entry)."""
    scene, frame, params, _ = C.load_config(name)
    params.count_traversal = 1
    out = {}
    for b in (abi.RTX_BUILD_SAH_HOST, abi.RTX_BUILD_SAH_GPU):
        renderer.set_builder(b)
        renderer.upload(scene)
        rgb, z = renderer.render(frame, params)
        out[b] = (rgb, z, renderer.stats())
    a, za, sa = out[abi.RTX_BUILD_SAH_HOST]
    b, zb, sb = out[abi.RTX_BUILD_SAH_GPU]
    assert sb.builder == abi.RTX_BUILD_SAH_GPU
    for f in ("bvh_nodes", "bvh_prims", "bvh_depth", "wide_nodes", "wide_depth", "wide_entries", "shadow_walk",
              "closest_rays", "shadow_rays", "node_visits", "sphere_tests", "shadow_box_tests"):
        # per-ray work sums; wave-level counts (steps, leaf rounds) depend on which shade points share
        # a wave, i.e. on k_trace's emission order, which varies between runs
        assert getattr(sa, f) == getattr(sb, f), (name, f, getattr(sa, f), getattr(sb, f))
    # the triangle tests of both walks too (the any-hit walk stops at its first opaque hit, so its
    # count follows which primitive sits in which leaf slot: round 4's host partition was unstable
    # and put a rotated Menger face's two equal-centroid triangles in the other order)
    assert sa.tri_tests == sb.tri_tests and sa.shadow_tri_tests == sb.shadow_tri_tests, name
    assert np.array_equal(a, b) and np.array_equal(za, zb), name


@pytest.mark.parametrize("name", ["s5_path2", "s6_amb"])
def test_gpu_wave_counts_vary_only_with_packing(renderer, name):
    """The same scene and tree rendered twice: every per-ray traversal sum is identical, while the
    wave-level counts (wave steps, leaf rounds, uniform steps) may move a little, because k_trace
    appends shade points from its waves in completion order, so which points share a k_shadow wave
    varies (r03e: 108,865 vs 108,786 wave steps).  Images are bit-identical either way; the
    variation is pinned here at 1 %."""
    scene, frame, params, _ = C.load_config(name)
    params.count_traversal = 1
    renderer.set_builder(abi.RTX_BUILD_SAH_GPU)
    renderer.upload(scene)
    runs = []
    for _ in range(2):
        rgb, z = renderer.render(frame, params)
        runs.append((rgb, z, renderer.stats()))
    (a, za, sa), (b, zb, sb) = runs
    assert np.array_equal(a, b) and np.array_equal(za, zb)
    for f in ("closest_rays", "shadow_rays", "node_visits", "tri_tests", "sphere_tests", "shadow_box_tests",
              "shadow_tri_tests", "shade_points"):
        assert getattr(sa, f) == getattr(sb, f), (name, f)
    for f in ("shadow_wave_steps", "shadow_leaf_rounds", "shadow_uniform_steps", "shadow_wave_walks"):
        x, y = getattr(sa, f), getattr(sb, f)
        assert abs(x - y) <= 0.01 * max(x, y, 1), (name, f, x, y)


from tree_audit import wide_tree_diff  # noqa: E402  (the walk of two 8-wide trees in step)


@pytest.mark.parametrize("name", ["s5_path2", "s6_amb", "s3_path2", "st_amb"])
def test_gpu_sah_device_collapse_equals_host_collapse(renderer, name):
    """the device 8-wide collapse (rtx_wide8_dev.hip) of the device SAH tree makes the host
    collapse's tree (rtx_wide8.cpp) of the host SAH tree, entry for entry: same frames, slots,
    8-bit planes and leaf records (only the entry layout differs, breadth- vs depth-first)"""
    scene, _, _, _ = C.load_config(name)
    trees = {}
    for b in (abi.RTX_BUILD_SAH_HOST, abi.RTX_BUILD_SAH_GPU):
        renderer.set_builder(b)
        renderer.upload(scene)
        trees[b] = renderer.wide_tree()
    (ta, fa), (tb, fb) = trees[abi.RTX_BUILD_SAH_HOST], trees[abi.RTX_BUILD_SAH_GPU]
    assert len(ta) == len(tb), (name, len(ta), len(tb))
    if not len(ta):  # small scenes walk the threaded BVH2 or no tree at all: no 8-wide tree built
        return
    assert np.array_equal(fa, fb), (fa, fb)
    diffs = wide_tree_diff(ta, tb)
    assert not diffs, (name, len(diffs), diffs[:8])
