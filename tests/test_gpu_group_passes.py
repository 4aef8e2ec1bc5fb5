"""Multi-pass and adaptive rendering on device groups (rtx_group_render_passes, rtx_group_render_adaptive,
csrc/rtx_group_passes.cpp) on the one-GPU box.

The reference is always the single context in the same test (Renderer.render_adaptive, Renderer.render_passes): the
group folds, selects and outputs with the single context's own kernels on state addressed by the global tile index, so
its results are the single context's bit for bit for any number of members, and no tolerance enters but the one
test_gpu_adaptive.py already uses between render_adaptive and render_passes (2 float ulps, 1e-9 on the error).  The
groups are loopback groups (n contexts on one device; the exchanges are device-to-device copies) and the group of one
that sends to itself over RCCL (rccl_self), whose receive buffers are filled with 0xFF beforehand.  The target tau is
taken as test_gpu_adaptive.py takes it: the error render_passes reports after 8 full passes.

NOT exercised here: RCCL between distinct devices (this box has one GPU).
"""
import ctypes
import os

import numpy as np
import pytest

import conftest as C
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

SEED = 11
PATH = ["-g", "path", "-n", "1"]
MODES = {"plain": {}, "jitter": {"jitter": True}}
SCENES = {"scene1": "scene1.json", "scene5_standin": "scene5_standin.json"}
PASSES, MIN_PASSES = 24, 3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dbits(x):
    return np.float64(x).view(np.uint64)


def path_params(**kw):
    return rtxpy.params_from_args(PATH, **{"seed": SEED, **kw})


def within_ulps(got, want, ulps=2):
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulps * np.spacing(np.abs(want)).astype(np.float64))


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def stat_tuple(s):
    return tuple(getattr(s, f) for f, _ in s._fields_)


class World:
    """the scenes, one single context per scene with its reference runs made once, and one group per size, which
    uploads a scene again only when the test before it used another"""

    def __init__(self):
        self.scenes, self.ctx, self.taus, self.refs, self.groups = {}, {}, {}, {}, {}

    def scene(self, name):
        if name not in self.scenes:
            if "standin" in name:
                import standins
                standins.ensure_scene(name.split("_standin")[0])
            self.scenes[name] = rtxpy.Scene.load(os.path.join(C.SCENES, SCENES[name]), base_dir=C.GOLDEN)
        return self.scenes[name]

    def renderer(self, name):
        if name not in self.ctx:
            r = rtxpy.Renderer(0)
            r.upload(self.scene(name))
            self.ctx[name] = r
        return self.ctx[name], self.scene(name)

    def tau(self, name, w, h, mode):
        """the error rtx_render_passes reports after 8 full passes"""
        key = (name, w, h, mode)
        if key not in self.taus:
            r, scene = self.renderer(name)
            r.render_passes(scene.frame(w, h), path_params(), 8, **MODES[mode])
            self.taus[key] = float(np.float32(r.pass_stats().error)) or 1e-3
        return self.taus[key]

    def adaptive(self, name, w, h, mode):
        """the single context's adaptive run: (tau, (rgb, z, var, n_t), stats); nothing changes the arrays"""
        key = (name, w, h, mode)
        if key not in self.refs:
            r, scene = self.renderer(name)
            tau = self.tau(name, w, h, mode)
            out = r.render_adaptive(scene.frame(w, h), path_params(), PASSES, tau, min_passes=MIN_PASSES, **MODES[mode])
            self.refs[key] = (tau, out, r.adaptive_stats())
        return self.refs[key]

    def group(self, kind, name):
        """kind: an int n (loopback group of n), "one" (rtx_group_open of one device) or "self" (rccl_self)"""
        if kind not in self.groups:
            if kind == "one":
                g = rtxpy.Group([0])
            elif kind == "self":
                g = rtxpy.Group([0], rccl_self=True)
            else:
                g = rtxpy.Group([0], loopback=kind)
            self.groups[kind] = [g, None]
        g, have = self.groups[kind]
        if have != name:
            g.upload(self.scene(name))
            self.groups[kind][1] = name
        return g

    def close(self):
        for g, _ in self.groups.values():
            g.close()
        for r in self.ctx.values():
            r.close()
        for s in self.scenes.values():
            s.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def check_adaptive(world, kind, name, w, h, mode):
    """the group's adaptive run against the single context's: every output's bits, every count, the error's bits"""
    tau, want, sw = world.adaptive(name, w, h, mode)
    g = world.group(kind, name)
    got = g.render_adaptive(world.scene(name).frame(w, h), path_params(), PASSES, tau, min_passes=MIN_PASSES, **MODES[mode])
    sg = g.adaptive_stats()
    n_t = want[3]
    print(f"{name} {w}x{h} {mode} group {kind}: R {sw.passes_run}, sum n_t {int(n_t.sum())} of {sw.passes_run * n_t.size}, "
          f"error {sw.error:.6g} / {sg.error:.6g}, exchanges {g.exchange_stats().exchanges}, bytes {g.exchange_stats().bytes}")
    for x, y, what in zip(got, want, ("rgb", "z", "variance", "tile_passes")):
        assert np.array_equal(bits(x), bits(y)), what
    assert (sg.passes_run, sg.tiles, sg.tile_passes) == (sw.passes_run, sw.tiles, sw.tile_passes) == \
        (int(n_t.max()), n_t.size, int(n_t.sum()))
    assert dbits(sg.error) == dbits(sw.error)
    assert (sg.closest_rays, sg.shadow_rays) == (sw.closest_rays, sw.shadow_rays)
    assert sg.render_ms > 0 and sg.fold_ms > 0
    return got, sg, g


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("name,w,h", [("scene1", 64, 64), ("scene5_standin", 64, 40)])
def test_adaptive_on_a_loopback_group_is_the_single_context(world, name, w, h, n, mode):
    _, want, sw = world.adaptive(name, w, h, mode)
    assert want[3].min() < want[3].max()  # the run decided something: tiles stopped at different passes
    _, _, g = check_adaptive(world, n, name, w, h, mode)
    ex = g.exchange_stats()
    T = want[3].size
    assert ex.exchanges == sw.passes_run and ex.exchange_ms > 0 and ex.gather_ms > 0
    # at least every pass's statistics of the members that travel, and their records
    travelling = sum(len(range(r, T, n)) for r in range(1, n))
    assert ex.bytes >= sw.passes_run * travelling * 24 + travelling * 64 * 32


def test_a_member_that_falls_idle(world):
    """scene1 at 64x64 on 8 members: tiles_x = 8, so a member owns a tile column, and a column whose tiles have all
    stopped before the run ends leaves its member with nothing to render while the others go on"""
    _, want, sw = world.adaptive("scene1", 64, 64, "jitter")
    n_t, R = want[3].ravel(), sw.passes_run
    idle = [r for r in range(8) if n_t[r::8].max() < R]
    print("passes per member's column:", [int(n_t[r::8].max()) for r in range(8)], "R", R)
    assert idle, "no member of 8 falls idle before the last pass"
    check_adaptive(world, 8, "scene1", 64, 64, "jitter")


def test_more_than_256_active_tiles(world):
    """136x136 = 289 tiles on 3 members: the list filter runs a second round, the scatter a second block"""
    _, want, _ = world.adaptive("scene1", 136, 136, "jitter")
    assert want[3].size == 289
    check_adaptive(world, 3, "scene1", 136, 136, "jitter")


@pytest.mark.parametrize("w,h,n", [(17, 9, 8), (20, 61, 5), (1, 1, 2)])
def test_ragged_and_starved(world, w, h, n):
    """6 tiles on 8 members (two own nothing), 24 tiles cut by both edges on 5, one pixel on 2"""
    check_adaptive(world, n, "scene1", w, h, "jitter")


def test_plain_passes_on_groups_of_one_and_three(world):
    r, scene = world.renderer("scene1")
    frame, K = scene.frame(37, 29), 5
    ad = r.render_adaptive(frame, path_params(), K, 1e-6, min_passes=K, jitter=True)  # every tile receives every pass
    assert np.all(ad[3] == K)
    sa = r.adaptive_stats()
    want = r.render_passes(frame, path_params(), K, jitter=True)
    ps = r.pass_stats()
    runs = {}
    for kind in ("one", 3):
        g = world.group(kind, "scene1")
        got = g.render_passes(frame, path_params(), K, jitter=True)
        sg, ex = g.pass_stats(), g.exchange_stats()
        runs[kind] = (got, sg)
        # the same kernels as render_adaptive: the same bits
        assert same_bits(got, ad[:3]), kind
        assert dbits(sg.error) == dbits(sa.error)
        # render_passes folds pixel-major and sums the error block-strided: one float rounding, double rounding
        assert within_ulps(got[0], want[0]) and within_ulps(got[2], want[2])
        assert np.array_equal(bits(got[1]), bits(want[1]))
        assert abs(sg.error - ps.error) <= 1e-9 * ps.error and ps.error > 0
        assert (sg.passes_run, sg.closest_rays, sg.shadow_rays) == (K, ps.closest_rays, ps.shadow_rays)
        assert sg.render_ms > 0 and sg.accum_ms > 0
        # no target: the statistics travel once, after the last pass; a group of one moves nothing
        assert (ex.exchanges, ex.bytes > 0) == ((1, True) if kind == 3 else (0, False))
    assert same_bits(runs["one"][0], runs[3][0])
    assert stat_tuple(runs["one"][1])[:2] == stat_tuple(runs[3][1])[:2] and dbits(runs["one"][1].error) == dbits(runs[3][1].error)


def test_stopping_rule(world):
    r, scene = world.renderer("scene1")
    frame, m = scene.frame(64, 64), 5
    errs = []
    for k in (m, m + 1):
        r.render_passes(frame, path_params(), k, jitter=True)
        errs.append(r.pass_stats().error)
    target = float(np.float32(np.sqrt(errs[0] * errs[1])))
    assert errs[0] > target > errs[1]
    want = r.render_passes(frame, path_params(), PASSES, jitter=True, target_error=target, min_passes=2)
    assert r.pass_stats().passes_run == m + 1
    g = world.group(3, "scene1")
    got = g.render_passes(frame, path_params(), PASSES, jitter=True, target_error=target, min_passes=2)
    sg, ex = g.pass_stats(), g.exchange_stats()
    assert sg.passes_run == m + 1 and ex.exchanges == m  # looked at after passes 2 .. m + 1
    assert abs(sg.error - errs[1]) <= 1e-9 * errs[1]
    assert within_ulps(got[0], want[0]) and within_ulps(got[2], want[2]) and np.array_equal(bits(got[1]), bits(want[1]))


def test_rccl_self_group(world):
    """the RCCL calls on one GPU: the statistics, the list and the final records sent to itself into 0xFF-filled
    buffers, so the bits are the single context's only if RCCL delivered them all"""
    _, _, g = check_adaptive(world, "self", "scene1", 64, 64, "jitter")
    _, _, sw = world.adaptive("scene1", 64, 64, "jitter")
    ex = g.exchange_stats()
    assert ex.exchanges == sw.passes_run and ex.bytes >= sw.passes_run * 64 * 24 + 64 * 64 * 32
    r, scene = world.renderer("scene1")
    frame = scene.frame(37, 29)
    ad = r.render_adaptive(frame, path_params(), 4, 1e-6, min_passes=4, jitter=True)
    got = g.render_passes(frame, path_params(), 4, jitter=True)
    assert same_bits(got, ad[:3]) and dbits(g.pass_stats().error) == dbits(r.adaptive_stats().error)
    ex = g.exchange_stats()
    assert ex.exchanges == 1 and ex.bytes == 20 * 24 + 20 * 64 * 32


def test_two_runs_and_a_render_between(world):
    r, scene = world.renderer("scene1")
    frame = scene.frame(64, 64)
    a, sa, g = check_adaptive(world, 3, "scene1", 64, 64, "jitter")
    single = r.render(frame, path_params())
    between = g.render(frame, path_params())
    assert same_bits(between, single)
    b, sb, _ = check_adaptive(world, 3, "scene1", 64, 64, "jitter")
    assert same_bits(a, b)
    assert (sa.passes_run, sa.tile_passes, dbits(sa.error), sa.closest_rays, sa.shadow_rays) == \
        (sb.passes_run, sb.tile_passes, dbits(sb.error), sb.closest_rays, sb.shadow_rays)
    p1 = g.render_passes(frame, path_params(), 4, jitter=True)
    s1 = g.pass_stats()
    p2 = g.render_passes(frame, path_params(), 4, jitter=True)
    s2 = g.pass_stats()
    assert same_bits(p1, p2) and (s1.passes_run, dbits(s1.error), s1.closest_rays, s1.shadow_rays) == \
        (s2.passes_run, dbits(s2.error), s2.closest_rays, s2.shadow_rays)


def test_refusals_leave_the_statistics_and_the_group(world):
    scene = world.scene("scene1")
    frame = scene.frame(64, 64)
    fresh = rtxpy.Group([0], loopback=2)
    try:
        for call in (lambda: fresh.render_passes(frame, path_params(), 4), lambda: fresh.render_adaptive(frame, path_params(), 4, 0.01)):
            with pytest.raises(rtxpy.RtxError) as e:
                call()
            assert e.value.code == abi.RTX_ERR_STATE
        assert stat_tuple(fresh.pass_stats()) == stat_tuple(abi.PassStats())
    finally:
        fresh.close()
    g = world.group(3, "scene1")
    before = g.render_adaptive(frame, path_params(), 4, 1e30)
    g.render_passes(frame, path_params(), 3)
    kept = [stat_tuple(s) for s in (g.adaptive_stats(), g.pass_stats(), g.exchange_stats())]
    assert kept[0][:3] == (2, 64, 128) and kept[1][0] == 3
    refused = [lambda: g.render_adaptive(frame, path_params(tile_stride=2), 4, 0.01),
               lambda: g.render_adaptive(frame, path_params(tile_stride=2, tile_offset=1), 4, 0.01),
               lambda: g.render_passes(frame, path_params(tile_stride=2), 4),
               lambda: g.render_adaptive(frame, path_params(), 4, 0.0),
               lambda: g.render_adaptive(frame, path_params(), 4, 0.01, min_passes=1),
               lambda: g.render_adaptive(frame, path_params(), 4, 0.01, min_passes=5),
               lambda: g.render_passes(frame, path_params(), 4, target_error=0.01, min_passes=5),
               lambda: g.render_passes(frame, path_params(), 0)]
    for i, call in enumerate(refused):
        with pytest.raises(rtxpy.RtxError) as e:
            call()
        assert e.value.code == abi.RTX_ERR_ARG, i
    assert [stat_tuple(s) for s in (g.adaptive_stats(), g.pass_stats(), g.exchange_stats())] == kept
    after = g.render_adaptive(frame, path_params(), 4, 1e30)
    assert same_bits(after, before)
    # NULL outputs: each alone, and none
    pp = rtxpy.pass_params(passes=4, target_error=1e30)
    p = path_params()
    f, q, o = ctypes.byref(frame), ctypes.byref(p), ctypes.byref(pp)
    for keep in range(4):
        out = [np.full(x.shape, 0x7FE5C3E1, np.uint32).view(x.dtype) for x in before]
        ptr = [x.ctypes.data if i == keep else None for i, x in enumerate(out)]
        assert g.lib.rtx_group_render_adaptive(g._g, f, q, o, *ptr) == abi.RTX_OK
        assert np.array_equal(bits(out[keep]), bits(before[keep]))
    assert g.lib.rtx_group_render_adaptive(g._g, f, q, o, None, None, None, None) == abi.RTX_OK
    assert g.lib.rtx_group_render_passes(g._g, f, q, o, None, None, None) == abi.RTX_OK


def test_pass_record_device_kernels(world):
    import torch
    r, scene = world.renderer("scene1")
    rgb, z, var, _ = r.render_adaptive(scene.frame(37, 29), path_params(), 4, 1e-6, min_passes=4, jitter=True)
    var = var.copy()
    var.view(np.uint32)[0, 0] = (0x7FC00001, 0x80000000, 0xFFFFFFFF)  # a NaN with a payload, -0.0
    h, w = z.shape
    d_in = [torch.from_numpy(a.copy()).cuda() for a in (rgb, z, var)]
    d_out = [torch.full_like(a, 7.5) for a in d_in]
    lib, n, guard = rtxpy.rtx_lib(), 3, 64
    torch.cuda.synchronize()
    for k in range(n):
        cnt = lib.rtx_tile_pack_count(w, h, k, n)
        d_rec = torch.full((cnt + guard, 8), 7.5, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rtxpy._check(lib.rtx_pass_pack_device(r._ctx, *[a.data_ptr() for a in d_in], w, h, k, n, d_rec.data_ptr(), None))
        host = d_rec.cpu().numpy()
        assert np.array_equal(bits(host[:cnt]), bits(rtxpy.pass_pack(rgb, z, var, k, n)))
        assert np.all(host[cnt:] == 7.5)  # the guard records right after the shard's
        rtxpy._check(lib.rtx_pass_unpack_device(r._ctx, d_rec.data_ptr(), w, h, k, n, *[a.data_ptr() for a in d_out], None))
    torch.cuda.synchronize()
    for got, wantarr in zip(d_out, (rgb, z, var)):
        assert np.array_equal(bits(got.cpu().numpy()), bits(wantarr))
    # null outputs are skipped
    only_z = torch.full_like(d_in[1], 7.5)
    d_rec = torch.from_numpy(rtxpy.pass_pack(rgb, z, var, 0, 1)).cuda()
    torch.cuda.synchronize()
    rtxpy._check(lib.rtx_pass_unpack_device(r._ctx, d_rec.data_ptr(), w, h, 0, 1, None, only_z.data_ptr(), None, None))
    assert np.array_equal(bits(only_z.cpu().numpy()), bits(z))
