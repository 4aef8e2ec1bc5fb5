"""The trees rtx_upload_scene builds, audited structurally (tree_audit.py) on the catalogue of
hard_meshes.py: every box on the path to a primitive contains it, in the float BVH2, its threaded 16-bit copy
and the 8-wide compressed tree, for the four builders, both tree frames and leaves of 1 and 4.  No render and
no tolerance: integer structure, and float64 containment with slack >= 0.

Run with -s for the measured figures (profiles/treeaudit/README.md)."""
import numpy as np
import pytest

import hard_meshes as HM
import rays_exhaustive as RX
import tree_audit as TA
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

BUILDERS = {"sahhost": abi.RTX_BUILD_SAH_HOST, "sahgpu": abi.RTX_BUILD_SAH_GPU, "lbvh": abi.RTX_BUILD_LBVH_GPU,
            "ploc": abi.RTX_BUILD_PLOC_GPU}
FRAMES = {"auto": abi.RTX_FRAME_AUTO, "world": abi.RTX_FRAME_WORLD}
LEAVES = (1, 4)


class Gpu:
    def __init__(self, tmp):
        self.paths = HM.write_scenes(tmp)
        self.loaded = {}

    def get(self, name):
        """(scene, records, transparent per object, emitters, tree frame under RTX_FRAME_AUTO)"""
        if name not in self.loaded:
            scene = HM.load(name, self.paths[name])
            objs = RX.objects_of(scene)
            self.loaded[name] = (scene, objs, HM.transparent_of(scene, objs), HM.emitters_of(scene), rtxpy.tree_frame(scene))
        return self.loaded[name]

    def close(self):
        for s in self.loaded.values():
            s[0].close()


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    g = Gpu(tmp_path_factory.mktemp("tree_audit_gpu"))
    yield g
    g.close()


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
    renderer.set_option(abi.RTX_OPT_TREE_FRAME, abi.RTX_FRAME_AUTO)


def upload(r, scene, builder, frame, leaf, walk):
    r.set_builder(BUILDERS[builder])
    r.set_option(abi.RTX_OPT_TREE_FRAME, FRAMES[frame])
    r.set_option(abi.RTX_OPT_BVH_LEAF, leaf)
    r.set_option(abi.RTX_OPT_SHADOW_WALK, walk)
    r.upload(scene)
    return r.stats()


def frame_of(st, auto_frame):
    """R, c of the frame the upload's trees are in: rtx_tree_frame's when the trees are rotated, else the identity"""
    if not st.tree_rotated:
        return np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    rotated, R, c, _ = auto_frame
    assert rotated
    return R, c


def inner_levels(st, builder, nnodes):
    """the inner nodes above the deepest leaf, from stats.bvh_depth: the SAH builders count the leaves' level too
    (bvh_build.cpp builds its root at depth 1, rtx_sah_build adds 1 where it built inner nodes), the LBVH and PLOC
    builders count the kept inner nodes on the way to the root (k_lb_depth, k_pl_leafpos)"""
    if builder in ("sahhost", "sahgpu") and (nnodes or (builder == "sahhost" and st.bvh_prims)):
        return st.bvh_depth - 1
    return st.bvh_depth


def where(fig):
    at = fig["min_slack_at"]
    return "-" if at is None else "level %d %s %s" % (at["level"], at["axis"], at["side"])


@pytest.mark.parametrize("name", HM.SCENES)
def test_every_box_contains_its_primitives(gpu, renderer, name):
    scene, objs, transparent, emitters, auto_frame = gpu.get(name)
    nb = int(HM.is_bounded(objs).sum())
    for builder in BUILDERS:
        for frame in FRAMES:
            for leaf in LEAVES:
                what = (name, builder, frame, leaf)
                st = upload(renderer, scene, builder, frame, leaf, abi.RTX_WALK_W8)
                if frame == "world":
                    assert st.tree_rotated == 0
                R, c = frame_of(st, auto_frame)
                b = renderer.bvh2()
                assert len(b["prims"]) == nb == st.bvh_prims and len(b["nodes"]) == st.bvh_nodes, what
                assert len(b["qnodes"]) == 0, what  # (the shadow walk takes the 8-wide tree, or there is nothing to walk)
                rep2 = TA.audit_bvh2(b["nodes"], b["prims"], b["root_ref"], objs, R, c, max_leaf=leaf, transparent=transparent,
                                     depth=inner_levels(st, builder, len(b["nodes"])))
                assert not rep2.violations, (what, "BVH2", len(rep2.violations), rep2.violations[:6])
                ent, qf = renderer.wide_tree()
                if nb - len(emitters) == 0:
                    assert b["root_ref"] == TA.EMPTY_REF and len(ent) == 0 and st.wide_nodes == 0, what
                    continue
                assert st.shadow_walk == abi.RTX_WALK_W8 and len(ent) == st.wide_entries > 0, what
                rep = TA.audit_wide(ent, qf, objs, R, c, emitters, transparent=transparent, prims=b["prims"], stats=st)
                assert not rep.violations, (what, "8-wide", len(rep.violations), rep.violations[:6])
                f, f2 = rep.figures, rep2.figures
                assert f["min_slack"] >= 0 and f["max_exponent"] <= TA.MAX_EXPONENT and f2["min_slack"] >= 0
                assert f["leaves"] == nb - len(emitters)
                print("AUDIT | %s | %s | %s | %d | %d | %d | %d | %d | %d | %.4g | %s | %d of %d | %.3g | %d" % (
                    name, builder, frame, leaf, nb, st.bvh_depth, st.wide_depth, st.wide_nodes, f["max_exponent"], f["min_slack"],
                    where(f), f["clamped"], f["boxes"], f2["min_slack"], st.tree_rotated))


@pytest.mark.parametrize("name", HM.SCENES)
def test_threaded_copy_is_a_preorder_of_containing_boxes(gpu, renderer, name):
    scene, objs, transparent, emitters, auto_frame = gpu.get(name)
    nb = int(HM.is_bounded(objs).sum())
    for builder in BUILDERS:
        for frame in FRAMES:
            for leaf in LEAVES:
                what = (name, builder, frame, leaf)
                st = upload(renderer, scene, builder, frame, leaf, abi.RTX_WALK_BVH2)
                R, c = frame_of(st, auto_frame)
                b = renderer.bvh2()
                assert len(renderer.wide_tree()[0]) == 0 and st.wide_nodes == 0, what
                if not nb:
                    assert len(b["qnodes"]) == 0 and b["root_ref"] == TA.EMPTY_REF, what
                    continue
                assert st.shadow_walk == abi.RTX_WALK_BVH2 and len(b["qnodes"]) == len(b["nodes"]) + (len(b["nodes"]) + 1), what
                rep = TA.audit_threaded(b["qnodes"], b["qframe"], len(b["nodes"]), b["prims"], objs, R, c)
                assert not rep.violations, (what, "threaded", len(rep.violations), rep.violations[:6])
                assert rep.figures["depth"] == inner_levels(st, builder, len(b["nodes"])) and rep.figures["min_slack"] >= 0, what
                rep2 = TA.audit_bvh2(b["nodes"], b["prims"], b["root_ref"], objs, R, c, max_leaf=leaf, transparent=transparent,
                                     depth=inner_levels(st, builder, len(b["nodes"])))
                assert not rep2.violations, (what, "BVH2", len(rep2.violations), rep2.violations[:6])
                f = rep.figures
                print("THREADED | %s | %s | %s | %d | %d | %d | %.4g | %s | %d" % (name, builder, frame, leaf, f["qnodes"], f["depth"],
                                                                                 f["min_slack"], where(f), f["clamped"]))


# Where the depth budget forces a median split the host builder partitions by centroid (nth_element) and the
# device takes the middle of the range; no scene of the catalogue is deep enough to get there.
HOST_DEVICE_EXEMPT = {}


@pytest.mark.parametrize("name", HM.SCENES)
def test_host_and_device_sah_trees_agree(gpu, renderer, name):
    scene, objs, _, emitters, _ = gpu.get(name)
    trees = {}
    for builder in ("sahhost", "sahgpu"):
        st = upload(renderer, scene, builder, "auto", 1, abi.RTX_WALK_W8)
        trees[builder] = renderer.wide_tree() + (inner_levels(st, builder, st.bvh_nodes), st.bvh_nodes, st.wide_depth, st.wide_nodes)
    (ta, fa, *sa), (tb, fb, *sb) = trees["sahhost"], trees["sahgpu"]
    if name in HOST_DEVICE_EXEMPT:
        return
    assert sa == sb, (name, sa, sb)
    assert len(ta) == len(tb), (name, len(ta), len(tb))
    if not len(ta):
        assert int(HM.is_bounded(objs).sum()) - len(emitters) == 0
        return
    assert np.array_equal(fa, fb), (fa, fb)
    diffs = TA.wide_tree_diff(ta, tb)
    assert not diffs, (name, len(diffs), diffs[:8])


def test_coincident_primitives_build_balanced_trees(gpu, renderer):
    """600 copies of one triangle: every builder splits or merges them evenly (the SAH builders and LBVH by index,
    PLOC by its order of tied pairs), within two levels of ceil(log2 600) = 10; by the lower pair index alone
    PLOC merged one pair a round into a chain 599 deep"""
    scene, objs, _, _, _ = gpu.get("dupes")
    for builder in BUILDERS:
        st = upload(renderer, scene, builder, "auto", 1, abi.RTX_WALK_W8)
        depth = inner_levels(st, builder, st.bvh_nodes)
        print("dupes", builder, "inner levels", depth, "wide depth", st.wide_depth)
        assert 10 <= depth <= 12 and st.wide_depth <= 8, (builder, depth, st.wide_depth)


def test_walk_selection_at_the_boundaries(gpu, renderer):
    want = {0: abi.RTX_WALK_BVH2, 1: abi.RTX_WALK_LINEAR, 2: abi.RTX_WALK_LINEAR, 8: abi.RTX_WALK_LINEAR, 9: abi.RTX_WALK_BVH2,
            1024: abi.RTX_WALK_BVH2, 1025: abi.RTX_WALK_W8}
    assert abi.RTX_SHADOW_LINEAR_MAX == 8 and set(want) == set(HM.COUNTS)
    for n in HM.COUNTS:
        scene, objs, _, _, _ = gpu.get("count%d" % n)
        for builder in BUILDERS:
            st = upload(renderer, scene, builder, "auto", 1, abi.RTX_WALK_AUTO)
            assert st.shadow_walk == want[n] and st.bvh_prims == n, (n, builder, st.shadow_walk)
            b = renderer.bvh2()
            assert (len(b["qnodes"]) > 0) == (want[n] == abi.RTX_WALK_BVH2 and n > 0), (n, builder)
            assert (st.wide_nodes > 0) == (want[n] == abi.RTX_WALK_W8), (n, builder)


def test_read_bvh2_before_an_upload_fails():
    import ctypes
    r = rtxpy.Renderer(0)
    try:
        n = [ctypes.c_uint32(7) for _ in range(4)]
        rc = r.lib.rtx_read_bvh2(r._ctx, None, 0, ctypes.byref(n[0]), ctypes.byref(n[1]), ctypes.byref(n[2]), None, 0,
                                 ctypes.byref(n[3]), None)
        assert rc == abi.RTX_ERR_STATE
        assert r.lib.rtx_read_bvh2(r._ctx, None, 0, None, None, None, None, 0, None, None) == abi.RTX_ERR_ARG
    finally:
        r.close()
