"""Tile-list renders on the GPU (rtx_render_tiles*, k_trace<.., LIST> / k_accum<LIST>).

A listed tile is the same tile of the full render bit for bit, every other pixel keeps the caller's bits, the ray
counts of a list and of its complement add up to the full render's, and the even tiles equal the arithmetic shard
0/2.  The same with small chunks and with the shade-point overflow retry, then the device entry with guard words
and a caller's stream, and the argument errors.
"""
import ctypes
import os

import numpy as np
import pytest

import conftest as C
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FE5C3E1  # a quiet NaN with a payload: no render writes these bits
SCENES = {"scene1": "scene1.json", "scene5_standin": "scene5_standin.json"}  # a linear walk, an 8-wide tree
PARAMS = {"ambient": [], "path": ["-g", "path", "-n", "1"]}
FRAMES = [(17, 33), (1, 1), (64, 64), (300, 2)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sentinel(shape):
    return np.full(shape, SENTINEL, np.uint32).view(np.float32)


def tile_mask(w, h, tiles):
    """(h, w) bool: the pixels of the listed tiles"""
    tx = (w + 7) // 8
    yy, xx = np.mgrid[0:h, 0:w]
    return np.isin((yy // 8) * tx + xx // 8, np.asarray(tiles, np.int64))


class World:
    def __init__(self):
        self.scenes, self.ctx, self.full = {}, {}, {}

    def renderer(self, name):
        if name not in self.ctx:
            if "standin" in name:
                import standins
                standins.ensure_scene(name.split("_standin")[0])
            self.scenes[name] = rtxpy.Scene.load(os.path.join(C.SCENES, SCENES[name]), base_dir=C.GOLDEN)
            r = rtxpy.Renderer(0)
            r.upload(self.scenes[name])
            self.ctx[name] = r
        return self.ctx[name], self.scenes[name]

    def whole(self, name, mode, w, h):
        """Renderer.render of the whole frame, once: (rgb, z, closest rays, shadow rays); nothing changes it"""
        key = (name, mode, w, h)
        if key not in self.full:
            r, scene = self.renderer(name)
            rgb, z = r.render(scene.frame(w, h), params(mode))
            st = r.stats()
            self.full[key] = (rgb, z, st.closest_rays, st.shadow_rays)
        return self.full[key]

    def close(self):
        for r in self.ctx.values():
            r.close()
        for s in self.scenes.values():
            s.close()


def params(mode, **kw):
    return rtxpy.params_from_args(PARAMS[mode], **{"seed": 5, **kw})


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def render_list(r, frame, p, tiles):
    """the list onto sentinel-filled buffers -> (rgb, z, closest rays, shadow rays)"""
    rgb, z = sentinel((frame.height, frame.width, 3)), sentinel((frame.height, frame.width))
    r.render_tiles(frame, p, tiles, rgb, z)
    st = r.stats()
    return rgb, z, st.closest_rays, st.shadow_rays


def check_list(got, full, w, h, tiles):
    """listed tiles: the full render's bits; every other pixel: the sentinel's"""
    m = tile_mask(w, h, tiles)
    for g, f in zip(got[:2], full[:2]):
        assert np.array_equal(bits(g)[m], bits(f)[m])
        assert np.all(bits(g)[~m] == SENTINEL)


def lists_of(T, seed):
    rng = np.random.default_rng(seed)
    sub = np.flatnonzero(rng.random(T) < 0.4).astype(np.uint32)
    return [np.zeros(0, np.uint32), np.array([0], np.uint32), np.array([T - 1], np.uint32), sub]


def check_frame(world, name, mode, w, h):
    r, scene = world.renderer(name)
    frame, p = scene.frame(w, h), params(mode)
    full = world.whole(name, mode, w, h)
    T = ((w + 7) // 8) * ((h + 7) // 8)
    every = np.arange(T, dtype=np.uint32)
    got = render_list(r, frame, p, every)
    assert np.array_equal(bits(got[0]), bits(full[0])) and np.array_equal(bits(got[1]), bits(full[1]))
    assert got[2:] == full[2:]
    for tiles in lists_of(T, 1000 * w + h):
        got = render_list(r, frame, p, tiles)
        check_list(got, full, w, h, tiles)
        if len(tiles) == 0:
            assert got[2:] == (0, 0)
        # a list and its complement trace the full render's rays between them
        rest = render_list(r, frame, p, np.setdiff1d(every, tiles).astype(np.uint32))
        assert got[2] + rest[2] == full[2] and got[3] + rest[3] == full[3]
    # the even tiles are the shard 0 / 2, rendered onto the same prefilled buffers
    rgb, z = sentinel((h, w, 3)), sentinel((h, w))
    r.render(frame, params(mode, tile_stride=2, tile_offset=0), rgb, z)
    st = r.stats()
    got = render_list(r, frame, p, every[::2])
    assert np.array_equal(bits(got[0]), bits(rgb)) and np.array_equal(bits(got[1]), bits(z))
    assert got[2:] == (st.closest_rays, st.shadow_rays)


@pytest.mark.parametrize("w,h", FRAMES)
@pytest.mark.parametrize("mode", sorted(PARAMS))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_listed_tiles_are_the_full_renders(world, name, mode, w, h):
    check_frame(world, name, mode, w, h)


@pytest.mark.parametrize("option,value", [(abi.RTX_OPT_CHUNK_TILES, 3), (abi.RTX_OPT_SP_PER_TILE, 1)])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_chunks_and_the_overflow_retry(world, name, option, value):
    """list positions in chunks of 3, and chunks sized for one shade point per tile, which overflow and halve: 576
    tiles, so that a list's shade points exceed one overflowing chunk's retry margin (as test_gpu_chunks)"""
    r, scene = world.renderer(name)
    w, h, T = 256, 144, 576
    frame, p = scene.frame(w, h), params("path")
    full = world.whole(name, "path", w, h)  # rendered before the option is set
    check_frame(world, name, "path", 17, 33)
    small = world.whole(name, "path", 17, 33)
    sub = lists_of(T, 7)[3]
    rest = np.setdiff1d(np.arange(T), sub).astype(np.uint32)
    r.set_option(option, value)
    try:
        check_frame(world, name, "path", 17, 33)
        a = render_list(r, frame, p, sub)
        chunks = r.stats().chunks
        assert chunks == -(-len(sub) // 3) if option == abi.RTX_OPT_CHUNK_TILES else chunks > 1
        b = render_list(r, frame, p, rest)
        assert r.stats().chunks > 1
    finally:
        r.set_option(option, 0)
    check_list(a, full, w, h, sub)
    check_list(b, full, w, h, rest)
    assert a[2] + b[2] == full[2] and a[3] + b[3] == full[3]
    assert small is world.whole(name, "path", 17, 33)


def test_the_estimate_of_a_full_render_survives_a_list_render(world):
    """a list render reads the shade points per tile the last full render saw and does not replace them: the full
    render after a one-tile list render is the full render before it, statistics' chunk count included"""
    r, scene = world.renderer("scene1")
    frame, p = scene.frame(64, 64), params("path")
    a = r.render(frame, p)
    sa = r.stats()
    render_list(r, frame, p, np.array([0], np.uint32))
    b = r.render(frame, p)
    sb = r.stats()
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    assert (sa.chunks, sa.closest_rays, sa.shadow_rays, sa.shade_points) == (sb.chunks, sb.closest_rays, sb.shadow_rays, sb.shade_points)


def test_device_entry_with_guard_words_and_a_stream(world):
    import torch
    r, scene = world.renderer("scene1")
    w, h, guard = 37, 29, 64
    frame, p = scene.frame(w, h), params("path")
    full = world.whole("scene1", "path", w, h)
    T = 5 * 4
    tiles = lists_of(T, 3)[3]
    n = w * h
    raw = np.full(guard + len(tiles) + guard, 0xFFFFFFFF, np.uint32)  # a guard entry would be out of range
    raw[guard:guard + len(tiles)] = tiles
    d_tiles = torch.from_numpy(raw.view(np.int32)).cuda()
    sent = float(np.array([SENTINEL], np.uint32).view(np.float32)[0])
    for stream in (None, torch.cuda.Stream()):
        bufs = [torch.full((guard + words + guard,), sent, dtype=torch.float32, device="cuda") for words in (3 * n, n)]
        torch.cuda.synchronize()
        r.render_tiles_device(frame, p, d_tiles.data_ptr() + 4 * guard, len(tiles), bufs[0].data_ptr() + 4 * guard,
                              bufs[1].data_ptr() + 4 * guard, stream=stream.cuda_stream if stream else None)
        st = r.stats()
        host = [b.cpu().numpy() for b in bufs]
        for b, words in zip(host, (3 * n, n)):
            assert np.all(bits(b[:guard]) == SENTINEL) and np.all(bits(b[guard + words:]) == SENTINEL)
        got = (host[0][guard:guard + 3 * n].reshape(h, w, 3), host[1][guard:guard + n].reshape(h, w))
        check_list(got, full, w, h, tiles)
        want = render_list(r, frame, p, tiles)
        assert (st.closest_rays, st.shadow_rays) == want[2:]
    assert np.array_equal(d_tiles.cpu().numpy().view(np.uint32), raw)
    # the device check: not increasing, out of range; nothing is written
    for bad in ([3, 3], [4, 2], [0, T], [T]):
        d_bad = torch.tensor(bad, dtype=torch.int32, device="cuda")
        buf = torch.full((3 * n,), sent, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(rtxpy.RtxError) as e:
            r.render_tiles_device(frame, p, d_bad.data_ptr(), len(bad), buf.data_ptr(), None)
        assert e.value.code == abi.RTX_ERR_ARG
        assert np.all(bits(buf.cpu().numpy()) == SENTINEL)
    r.render_tiles_device(frame, p, None, 0, None, None)  # no tile: nothing to do
    assert r.stats().closest_rays == 0


def test_argument_errors(world):
    r, scene = world.renderer("scene1")
    frame, p = scene.frame(17, 33), params("ambient")
    T = 15
    before = render_list(r, frame, p, [1, 2])
    for bad in ([0, 0], [2, 1], [T], [0, 5, T + 3], list(range(T)) + [T], [0xFFFFFFFF]):
        rgb = sentinel((33, 17, 3))
        with pytest.raises(rtxpy.RtxError) as e:
            r.render_tiles(frame, p, bad, rgb)
        assert e.value.code == abi.RTX_ERR_ARG, bad
        assert np.all(bits(rgb) == SENTINEL)
    f, q = ctypes.byref(frame), ctypes.byref(p)
    assert r.lib.rtx_render_tiles(r._ctx, f, q, None, 1, None, None) == abi.RTX_ERR_ARG  # a null list of one tile
    assert r.lib.rtx_render_tiles_device(r._ctx, f, q, None, 1, None, None, None) == abi.RTX_ERR_ARG
    assert r.lib.rtx_render_tiles(r._ctx, f, q, None, 0, None, None) == abi.RTX_OK
    for shard in (dict(tile_stride=2), dict(tile_stride=2, tile_offset=1), dict(tile_stride=0)):
        with pytest.raises(rtxpy.RtxError) as e:
            r.render_tiles(frame, params("ambient", **shard), [0])
        assert e.value.code == abi.RTX_ERR_ARG
    empty = abi.Frame.from_buffer_copy(bytes(frame))
    empty.height = 0
    with pytest.raises(rtxpy.RtxError) as e:
        r.render_tiles(empty, p, [])
    assert e.value.code == abi.RTX_ERR_ARG
    fresh = rtxpy.Renderer(0)
    try:
        with pytest.raises(rtxpy.RtxError) as e:
            fresh.render_tiles(frame, p, [0])
        assert e.value.code == abi.RTX_ERR_STATE
    finally:
        fresh.close()
    after = render_list(r, frame, p, [1, 2])  # the context is unharmed
    assert np.array_equal(bits(after[0]), bits(before[0])) and after[2:] == before[2:]
    # null outputs render and count
    assert r.lib.rtx_render_tiles(r._ctx, f, q, (ctypes.c_uint32 * 2)(1, 2), 2, None, None) == abi.RTX_OK
    st = r.stats()
    assert (st.closest_rays, st.shadow_rays) == before[2:]
