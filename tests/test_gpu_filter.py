"""Pixel reconstruction filters on the GPU (csrc/rtx_filter.hip through rtx_render_passes_filtered*).

A box of radius 1/2 is the plain fold, to the bit.  Every other filter against the float64 model of include/rtx.h
(tests/filter_model.py) run over the frames Renderer.render gives for rtx_pass_frame(k) and seed + k, with the
weights rtx_pass_filter_weights returns.  Then frame shapes that cut the halo, determinism, the device entry with
guard words, null outputs, the stopping rule against the model's own error, that the weights are used at all,
reconstruction quality against a filtered supersampled reference, and the argument errors.
"""
import ctypes

import numpy as np
import pytest

import filter_model as M
import rtxpy
import test_gpu_passes as P
from rtxpy import abi
from test_gpu_passes import bits, path_params

pytestmark = pytest.mark.gpu

MODES = {m: {"jitter": False, **P.MODES[m]} for m in ("plain", "jitter", "jitter+lens")}
# name -> (kind, radius, alpha); None: the library's default
FILTERS = {
    "tent 1": ("tent", 1.0, None),
    "tent 2.5": ("tent", 2.5, None),
    "gaussian": ("gaussian", None, None),
    "mitchell 2": ("mitchell", 2.0, None),
    "box 1.5": ("box", 1.5, None),
}


@pytest.fixture(scope="module")
def world():
    w = P.World()
    yield w
    w.close()


def filter_kw(name):
    kind, radius, alpha = FILTERS[name]
    return {"filter": kind, "radius": radius, "alpha": alpha}


def weights_of(name, mode, K):
    return [rtxpy.filter_weights(k, passes=K, **filter_kw(name), **MODES[mode]) for k in range(K)]


def close_to(got, want64, slack):
    """2 float ulps of the model's value plus the double state's share `slack`"""
    want = want64.astype(np.float32).astype(np.float64)
    tol = 2 * np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64) + slack
    return np.all(np.abs(got.astype(np.float64) - want) <= tol)


def check_against_model(world, scene, w, h, mode, K, filt):
    """render_passes_filtered against the float64 model over the K single renders.  The device's state is double
    and takes the model's operations in the model's order: its 25-term sums and K updates each carry a few 2^-53 of
    relative error, and what cancels under Mitchell's negative lobes is bounded by A_p = max_k sum |w c| / W_k.  So
    rgb is one float rounding of a mean within 2^-47 A_p, and the variance one of a value within 2^-44 A_p^2
    (derived, not measured)."""
    frames = [world.single(scene, w, h, mode, k) for k in range(K)]
    r = world.renderer(scene)
    rgb, z, var = r.render_passes_filtered(world.scene(scene).frame(w, h), path_params(), K, **filter_kw(filt), **MODES[mode])
    st = r.pass_stats()
    mean, m2, wsum, amp = M.fold([f[0] for f in frames], weights_of(filt, mode, K))
    want_var = M.variance_of(m2, wsum, K)
    assert st.passes_run == K
    assert np.array_equal(bits(z), bits(frames[0][1]))
    err_rgb = np.abs(rgb.astype(np.float64) - mean.astype(np.float32).astype(np.float64))
    err_var = np.abs(var.astype(np.float64) - want_var.astype(np.float32).astype(np.float64))
    print(f"{scene} {w}x{h} {mode} K={K} {filt}: max |rgb - model| = {err_rgb.max():.3g}, max |var - model| = {err_var.max():.3g}, "
          f"max A = {amp.max():.3g}")
    assert close_to(rgb, mean, 2.0 ** -47 * amp)
    if K == 1:
        assert not var.any() and st.error == 0.0
    else:
        assert close_to(var, want_var, 2.0 ** -44 * amp * amp)
        assert var.any()
        e = M.error_of(mean, want_var, K)
        assert abs(st.error - e) <= 1e-9 * e
    assert st.closest_rays == sum(f[2] for f in frames) and st.shadow_rays == sum(f[3] for f in frames)
    return rgb, z, var


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_box_half_is_the_plain_fold(world, mode, K):
    """one tap of weight 1 per pass: rgb, variance and z are rtx_render_passes's bits; the error differs by the
    partial sums' order only"""
    r, frame = world.renderer("scene1"), world.scene("scene1").frame(64, 64)
    plain = r.render_passes(frame, path_params(), K, **MODES[mode])
    sp = r.pass_stats()
    got = r.render_passes_filtered(frame, path_params(), K, filter="box", radius=0.5, **MODES[mode])
    sf = r.pass_stats()
    for x, y in zip(got, plain):
        assert np.array_equal(bits(x), bits(y))
    assert (sf.passes_run, sf.closest_rays, sf.shadow_rays) == (sp.passes_run, sp.closest_rays, sp.shadow_rays)
    assert abs(sf.error - sp.error) <= 1e-9 * sp.error
    assert (sf.error > 0) == (K > 1)


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("mode", ["jitter", "jitter+lens"])
@pytest.mark.parametrize("filt", sorted(FILTERS))
@pytest.mark.parametrize("scene,w,h", [("scene1", 64, 64), ("scenetest", 64, 36)])
def test_against_the_float64_model(world, scene, w, h, filt, mode, K):
    check_against_model(world, scene, w, h, mode, K, filt)


@pytest.mark.parametrize("filt", ["mitchell 2", "tent 2.5"])
@pytest.mark.parametrize("w,h", [(1, 1), (17, 33), (300, 2), (3, 70)])
def test_shapes(world, w, h, filt):
    """frames narrower or lower than the halo, tiles cut by the frame's edge, every border truncation: K = 3 with
    jitter and a lens"""
    check_against_model(world, "scene1", w, h, "jitter+lens", 3, filt)


def test_a_filter_without_jitter_is_a_blur(world):
    check_against_model(world, "scene1", 64, 64, "plain", 2, "gaussian")


def test_two_runs_give_the_same_bits(world):
    r, frame = world.renderer("scene1"), world.scene("scene1").frame(64, 64)
    for kw in ({}, {"target_error": 2.5e-3, "min_passes": 2}):
        a = r.render_passes_filtered(frame, path_params(), 6, filter="mitchell", radius=2.0, **kw)
        na = r.pass_stats()
        b = r.render_passes_filtered(frame, path_params(), 6, filter="mitchell", radius=2.0, **kw)
        nb = r.pass_stats()
        assert (na.passes_run, na.error) == (nb.passes_run, nb.error) and na.passes_run >= 2 and na.error > 0
        for x, y in zip(a, b):
            assert np.array_equal(bits(x), bits(y))


def test_device_entry_equals_the_host_entry_and_stays_in_bounds(world):
    import torch
    r, frame = world.renderer("scene1"), world.scene("scene1").frame(37, 29)
    n, guard = 37 * 29, 64
    kw = dict(filter="tent", radius=2.5, jitter=True, aperture=0.2, focus=4.0)
    want = r.render_passes_filtered(frame, path_params(), 3, **kw)
    bufs = [torch.full((words + guard,), 7.5, dtype=torch.float32, device="cuda") for words in (3 * n, n, 3 * n)]
    torch.cuda.synchronize()
    r.render_passes_filtered_device(frame, path_params(), 3, *[b.data_ptr() for b in bufs], **kw)
    for b, words, w in zip(bufs, (3 * n, n, 3 * n), want):
        host = b.cpu().numpy()
        assert np.array_equal(bits(host[:words]), bits(w).ravel())
        assert np.all(host[words:] == 7.5)  # the guard words right after the buffer
    # a stream of the caller's, and each output null in turn
    s = torch.cuda.Stream()
    for keep in range(3):
        d = torch.full((3 * n + guard,), 7.5, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ptr = [d.data_ptr() if i == keep else None for i in range(3)]
        r.render_passes_filtered_device(frame, path_params(), 3, *ptr, stream=s.cuda_stream, **kw)
        host = d.cpu().numpy()
        words = want[keep].size
        assert np.array_equal(bits(host[:words]), bits(want[keep]).ravel())
        assert np.all(host[words:] == 7.5)
    with pytest.raises(rtxpy.RtxError) as e:
        r.render_passes_filtered_device(frame, path_params(), 3, bufs[0].data_ptr() + 4, None, None, **kw)
    assert e.value.code == abi.RTX_ERR_ARG


def test_null_outputs(world):
    r, frame = world.renderer("scene1"), world.scene("scene1").frame(37, 29)
    want = r.render_passes_filtered(frame, path_params(), 3)
    pp, p, fp = rtxpy.pass_params(passes=3, jitter=True), path_params(), rtxpy.filter_params()
    args = (r._ctx, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(pp), ctypes.byref(fp))
    for keep in range(3):
        out = [np.full(w.shape, 7.5, np.float32) for w in want]
        ptr = [o.ctypes.data if i == keep else None for i, o in enumerate(out)]
        assert r.lib.rtx_render_passes_filtered(*args, *ptr) == abi.RTX_OK
        assert np.array_equal(bits(out[keep]), bits(want[keep]))
    assert r.lib.rtx_render_passes_filtered(*args, None, None, None) == abi.RTX_OK
    assert r.pass_stats().passes_run == 3


def test_stopping_rule(world):
    """the error after every pass from the model over the single renders; a target between two consecutive values
    (at least 1 % apart) stops exactly where the model's error first falls to it"""
    r, frame, K = world.renderer("scene1"), world.scene("scene1").frame(64, 64), 12
    frames = [world.single("scene1", 64, 64, "jitter", k)[0] for k in range(K)]
    ws = weights_of("gaussian", "jitter", K)
    E = []
    for n in range(1, K + 1):
        mean, m2, wsum, _ = M.fold(frames[:n], ws[:n])
        E.append(M.error_of(mean, M.variance_of(m2, wsum, n), n))  # E[n-1]: after n passes
    print("E after 1..12 filtered passes:", " ".join(f"{e:.6g}" for e in E))
    pair = next(i for i in range(3, K - 1) if abs(E[i] - E[i + 1]) >= 0.01 * max(E[i], E[i + 1]))
    target = float(np.float32(np.sqrt(E[pair] * E[pair + 1])))
    for min_passes in (2, 9):
        want_n = next((n for n in range(min_passes, K + 1) if E[n - 1] <= target), K)
        assert want_n < K  # the rule stops this run early
        got = r.render_passes_filtered(frame, path_params(), K, target_error=target, min_passes=min_passes)
        st = r.pass_stats()
        assert st.passes_run == want_n, (st.passes_run, want_n, min_passes)
        assert abs(st.error - E[want_n - 1]) <= 1e-9 * E[want_n - 1]
        whole = r.render_passes_filtered(frame, path_params(), want_n)
        for x, y in zip(got, whole):
            assert np.array_equal(bits(x), bits(y))
    r.render_passes_filtered(frame, path_params(), K, target_error=1e30, min_passes=3)
    assert r.pass_stats().passes_run == 3
    r.render_passes_filtered(frame, path_params(), K, target_error=0.0, min_passes=3)
    st = r.pass_stats()
    assert st.passes_run == K and abs(st.error - E[K - 1]) <= 1e-9 * E[K - 1]


def test_the_filtered_entry_differs_from_the_plain_one(world):
    """a kernel that ignored its weights would pass the box test"""
    r, frame = world.renderer("scene1"), world.scene("scene1").frame(64, 64)
    box = r.render_passes_filtered(frame, path_params(), 4, filter="box", radius=0.5)
    gauss = r.render_passes_filtered(frame, path_params(), 4)
    wide = r.render_passes_filtered(frame, path_params(), 4, radius=2.5, alpha=0.5)
    assert np.array_equal(bits(box[1]), bits(gauss[1]))  # z is pass 0's either way
    for a, b in ((box, gauss), (gauss, wide)):
        assert (bits(a[0]) != bits(b[0])).mean() > 0.5 and (bits(a[2]) != bits(b[2])).mean() > 0.5


# e(16 filtered jittered passes) / e(one ray) from the CPU oracle alone; the test's bound is 3x that
ORACLE_RATIO = {
    ("scene1", "gaussian"): 0.0041,
    ("scene3", "gaussian"): 0.0076,
    ("scenetest", "gaussian"): 0.0415,
    ("scene1", "mitchell 2"): 0.0068,
    ("scene3", "mitchell 2"): 0.0125,
    ("scenetest", "mitchell 2"): 0.0540,
}


FINE = {}


@pytest.mark.parametrize("filt", ["gaussian", "mitchell 2"])
@pytest.mark.parametrize("name,w,h", [("scene1", 64, 64), ("scene3", 64, 36), ("scenetest", 64, 36)])
def test_reconstruction_quality(world, name, w, h, filt):
    """noise-free frames (ambient GI, constant RNG).  The reference is the 8 x 8 supersampled frame reconstructed
    with the same filter in float64; e is the mean squared error against it.  The CPU oracle alone gives
    e(16 filtered jittered passes) / e(one ray) = ORACLE_RATIO: 0.0041 / 0.0076 / 0.0415 under the default Gaussian
    and 0.0068 / 0.0125 / 0.0540 under Mitchell 2 (scene1 / scene3 / scenetest; the one-pixel box of test_anti_aliasing
    gives 0.030 / 0.053 / 0.085 the same way), and the device the same six figures to the four decimals.  The bound
    is 3x the oracle's ratio, the margin test_anti_aliasing leaves for the device's float differences at edges."""
    r, frame = world.renderer(name), world.scene(name).frame(w, h)
    p = rtxpy.default_params(rng=abi.RTX_RNG_CONST)
    kind, radius, _ = FILTERS[filt]
    fp = rtxpy.filter_params(kind=kind) if radius is None else rtxpy.filter_params(kind=kind, radius=radius)
    if name not in FINE:  # the supersampled frame and the one-ray frame, rendered once per scene
        FINE[name] = (r.render(P.supersampled(frame, 8), p)[0], r.render(frame, p)[0])
    fine, one = FINE[name]
    ref = M.reconstruct(fine, 8, kind, float(fp.radius), float(fp.alpha))
    aa, _, _ = r.render_passes_filtered(frame, p, 16, filter=fp)
    e = lambda x: float(((x.astype(np.float64) - ref) ** 2).mean())  # noqa: E731
    ratio, bound = e(aa) / e(one), 3 * ORACLE_RATIO[(name, filt)]
    print(f"reconstruction {name} {w}x{h} {filt}: e(16 filtered passes) / e(one ray) = {ratio:.4f} (bound {bound:.4f}, "
          f"e(one ray) = {e(one):.4g})")
    assert bound < 1
    assert e(one) > 0 and ratio <= bound


def test_statistics_and_errors(world):
    r, scene = world.renderer("scene1"), world.scene("scene1")
    frame = scene.frame(64, 64)
    before, zb = r.render(frame, path_params())
    r.render_passes_filtered(frame, path_params(), 4)
    st, last = r.pass_stats(), r.stats()
    singles = [world.single("scene1", 64, 64, "jitter", k) for k in range(4)]
    assert st.passes_run == 4 and st.closest_rays == sum(s[2] for s in singles) and st.shadow_rays == sum(s[3] for s in singles)
    assert st.render_ms > 0 and st.accum_ms > 0 and st.error > 0
    assert (last.closest_rays, last.shadow_rays) == singles[3][2:]  # rtx_get_stats describes the last pass
    nan, inf = float("nan"), float("inf")
    bad_filters = [dict(kind=4), dict(kind="box", radius=0.25), dict(kind="box", radius=2.75), dict(kind="tent", radius=0.75),
                   dict(kind="gaussian", radius=0.5), dict(kind="mitchell", radius=3.0), dict(kind="tent", radius=nan),
                   dict(kind="gaussian", alpha=0.0), dict(kind="gaussian", alpha=-1.0), dict(kind="gaussian", alpha=inf),
                   dict(kind="gaussian", alpha=nan), dict(pad_=7)]
    for bad in bad_filters:
        with pytest.raises(rtxpy.RtxError) as e:
            r.render_passes_filtered(frame, path_params(), 2, filter=rtxpy.filter_params(**bad))
        assert e.value.code == abi.RTX_ERR_ARG, bad
    p, pp = path_params(), rtxpy.pass_params(passes=2, jitter=True)
    rgb = np.zeros((64, 64, 3), np.float32)
    assert r.lib.rtx_render_passes_filtered(r._ctx, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(pp), None, rgb.ctypes.data,
                                            None, None) == abi.RTX_ERR_ARG
    assert r.lib.rtx_render_passes_filtered_device(r._ctx, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(pp), None, None,
                                                   None, None, None) == abi.RTX_ERR_ARG
    # everything rtx_render_passes refuses
    for bad in (dict(tile_stride=2), dict(tile_stride=2, tile_offset=1), dict(tile_stride=0)):
        with pytest.raises(rtxpy.RtxError) as e:
            r.render_passes_filtered(frame, path_params(**bad), 2)
        assert e.value.code == abi.RTX_ERR_ARG
    for bad in (dict(passes=0), dict(passes=2, aperture=-1.0), dict(passes=2, target_error=0.1, min_passes=3)):
        with pytest.raises(rtxpy.RtxError) as e:
            r.render_passes_filtered(frame, path_params(), **bad)
        assert e.value.code == abi.RTX_ERR_ARG
    empty = abi.Frame.from_buffer_copy(bytes(frame))
    empty.width = 0
    with pytest.raises(rtxpy.RtxError) as e:
        r.render_passes_filtered(empty, path_params(), 2)
    assert e.value.code == abi.RTX_ERR_ARG
    fresh = rtxpy.Renderer(0)
    try:
        with pytest.raises(rtxpy.RtxError) as e:
            fresh.render_passes_filtered(frame, path_params(), 2)
        assert e.value.code == abi.RTX_ERR_STATE
    finally:
        fresh.close()
    # the context is left unharmed: the same frame as before, and the statistics of the refused calls' predecessor
    after, za = r.render(frame, path_params())
    assert np.array_equal(bits(after), bits(before)) and np.array_equal(bits(za), bits(zb))
    assert r.pass_stats().passes_run == 4
    # and the plain entry still gives what it gave: the two share the state buffer
    a = r.render_passes(frame, path_params(), 3, jitter=True)
    r.render_passes_filtered(frame, path_params(), 3)
    b = r.render_passes(frame, path_params(), 3, jitter=True)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
