"""k_shadow's sample order (rtx_shadow.hip order_begin) where its bookkeeping can go wrong: a lane keeps
its samples' buckets in registers (4 bits a packet, 16 packets at most), ranks them from ballots of the
buckets' bits, and a wave's slice holds the order and one 12-byte result record per sample; only the
records no lane will store are zeroed, and a slice is reused from run to run and from render to render
without being cleared.

 1. the order (RTX_KAT_ORDER) at the packet counts around a packet's and the registers' limits: still
    the stable sort of the samples that are not dark, with runs that are all dark, runs without a dark
    sample, and runs whose samples nearly all share a bucket;
 2. no stale slot: a long and a short run back to back in one slice, frames and counters equal with
    the option on and off;
 3. the same frame twice from one context, byte for byte.
"""
import numpy as np
import pytest

import order_model as M
import rtxpy
from rtxpy import abi
from test_gpu_order import check_equal, order_records, render_order
from test_gpu_premask import bench_params, edit_bench_scene

pytestmark = pytest.mark.gpu

# 65: a packet and a sample; 127 / 128 / 129: around two packets; 300: the bench scene's; 1023 / 1024: the
# sixteenth packet short of a sample and full (the last 4-bit field and the last "placed" bit)
SIZES = [65, 127, 128, 129, 300, 1023, 1024]


def check_records(x, y, nl):
    """every record's order is the stable sort of its lit samples by the device's buckets, which are the
    restatement's of the device's key values; returns the records' (lit, buckets) pairs"""
    out = []
    for i in range(len(x)):
        n_ord, npk = int(y[i, 0]), int(y[i, 1])
        order = y[i, 4:4 + M.CAP].astype(np.int64)
        buckets = y[i, 4 + M.CAP:4 + 2 * M.CAP].astype(np.int64)
        key = y[i, 4 + 2 * M.CAP:4 + 3 * M.CAP]
        assert npk == (nl + 63) // 64, (i, npk)
        assert (order[n_ord:] == -1).all() and (buckets[nl:] == M.BUCKETS).all(), i
        M.check_order(order[:n_ord], buckets, nl)
        lit = buckets[:nl] < M.BUCKETS
        assert n_ord == int(lit.sum()), (i, n_ord, int(lit.sum()))
        assert np.isfinite(key[:nl]).all(), i
        assert np.array_equal(buckets[:nl][lit], M.bucket(key[:nl][lit])), i
        out.append((lit, buckets[:nl]))
    return out


def all_dark_records(seed, n, nl, etype):
    """the normal points away from the emitter and ks = 0: no sample adds light, n_ord = 0"""
    x = order_records(seed, n, nl, etype)
    ec = x[:, 17:20] if etype == 0 else (x[:, 17:20] + x[:, 20:23] + x[:, 23:26]) / 3
    away = x[:, 0:3] - ec
    x[:, 3:6] = away / np.linalg.norm(away, axis=1, keepdims=True)
    x[:, 12:15] = 0.0
    return x


def horizon_records(seed, n, nl, etype):
    """the normal across the direction to the emitter's centre and ks = 0: the emitter straddles the
    point's horizon, so lit and dark samples interleave in every packet"""
    x = order_records(seed, n, nl, etype)
    ec = x[:, 17:20] if etype == 0 else (x[:, 17:20] + x[:, 20:23] + x[:, 23:26]) / 3
    across = np.cross(ec - x[:, 0:3], np.random.default_rng(seed).normal(size=(n, 3)))
    x[:, 3:6] = across / np.linalg.norm(across, axis=1, keepdims=True)
    x[:, 12:15] = 0.0
    return x


@pytest.mark.parametrize("etype", [0, 1])
@pytest.mark.parametrize("nl", SIZES)
def test_gpu_order_slots_sort_at_the_packing_limits(etype, nl):
    """random normals (a record's samples are mostly all lit or all dark), the box centre on the axis
    (the key's other direction), no dark sample (every lane placed in every packet), every sample dark
    (the run is skipped), and the emitter across the point's horizon (lit and dark samples interleave)"""
    x = np.concatenate([order_records(13 + nl, 4, nl, etype), order_records(17 + nl, 2, nl, etype, on_axis=True),
                        order_records(19 + nl, 2, nl, etype, dark=0), all_dark_records(23 + nl, 2, nl, etype),
                        horizon_records(31 + nl, 4, nl, etype)])
    y = rtxpy.gpu_kat(abi.KAT_ORDER, x)
    recs = check_records(x, y, nl)
    print("etype", etype, "nl", nl, "dark samples", [int((~lit).sum()) for lit, _ in recs])
    for lit, _ in recs[6:8]:  # dark = 0
        assert lit.all()
    mixed = [lit for lit, _ in recs[10:] if 0 < lit.sum() < nl]
    assert len(mixed) == 4  # a plane through a sphere's centre or a triangle's centroid has at least 4/9 of it on either side
    for i in (8, 9):  # all dark: the run is taken (its packets counted) and nothing is ordered
        assert not recs[i][0].any()
        assert int(y[i, 0]) == 0 and int(y[i, 1]) == (nl + 63) // 64
        assert (y[i, 4:4 + M.CAP] == -1).all()


@pytest.mark.parametrize("nl", [129, 1024])
def test_gpu_order_slots_rank_across_all_packets(nl):
    """a sliver triangle emitter set across the key's direction: the point at the origin, the emitter on
    the z axis, the box centre toward +x, so the key's direction is x and the sliver's long side runs
    along y.  A sliver's samples lie on a line through its centroid, the key's zero, so their key values
    are within 1e-3 of 0, the border of buckets 7 and 8: the samples share those two buckets (one alone
    cannot hold them), and either's rank runs across every packet of the run"""
    x = order_records(29, 3, nl, 1, dark=0)
    x[:, 0:3] = 0.0
    for i, eps in enumerate((1e-3, 1e-4, 0.0)):  # 0: a degenerate triangle, a segment
        x[i, 17:20] = [0.0, -1.0, 8.0]
        x[i, 20:23] = [0.0, 1.0, 8.0]
        x[i, 23:26] = [eps, 0.0, 8.0]
    x[:, 30:33] = [2.0, 0.0, 3.0]
    y = rtxpy.gpu_kat(abi.KAT_ORDER, x)
    for lit, buckets in check_records(x, y, nl):
        assert lit.all()
        used, counts = np.unique(buckets, return_counts=True)
        print("nl", nl, "buckets", used.tolist(), "samples", counts.tolist())
        assert set(used.tolist()) <= {7, 8}
        # the larger bucket has samples in every full packet of the run
        big = used[np.argmax(counts)]
        packets = set((np.flatnonzero(buckets == big) // 64).tolist())
        assert packets >= set(range(nl // 64)), sorted(packets)


def two_run_scene(tmp_path, lights):
    """the bench scene (its planes and the dragon stand-in, whose tree the points walk) with a small
    opaque occluder and two sphere emitters of `lights` samples, in that order"""
    def edit(d):
        objs = [o for o in d["Objects"] if "lights" not in o["parameters"]]
        objs.append({"type": "Sphere", "parameters": {"material": 0, "epsilon": 0.0003, "position": [-2.5, -1.2, 3.4], "radius": 0.35}})
        for n, pos, rad in zip(lights, ([-7.5, -4.0, 5.0], [5.5, -3.5, 1.5]), (0.5, 0.3)):
            objs.append({"type": "Sphere", "parameters": {"material": 2, "epsilon": 0.0003, "position": pos, "radius": rad, "lights": n}})
        d["Objects"] = objs
    return edit_bench_scene(tmp_path, "two_runs_%d_%d" % tuple(lights), edit)


@pytest.mark.parametrize("lights", [(1024, 65), (65, 1024)])
def test_gpu_order_slots_leave_nothing_stale(tmp_path, lights):
    """(1024, 65): every walking point orders a run of 16 packets and then one of a packet and a sample
    in the same slice; (65, 1024): the first emitter's one whole packet keeps the index order, a packet
    straddles the two, and the second's run is ordered from sample 128 on (961 samples).  Dark and lit
    samples interleave, so zeroed and stored records do.  Frames and every counter, with no tolerance"""
    scene = two_run_scene(tmp_path, lights)
    assert scene.desc.num_emitters == 2
    out = render_order(scene, scene.frame(64, 36), bench_params(2, 3), late=[(abi.RTX_OPT_SHADOW_SLOT, 64)])
    s, _ = check_equal(out)
    assert s.shadow_dark_rays > 0
    # both kinds of run were ordered: more ordered runs than one a point (1024, 65), or exactly one (65, 1024)
    print("lights", lights, "shade points", s.shade_points, "ordered runs", s.shadow_ordered_points)


def test_gpu_order_slots_same_frame_twice(tmp_path):
    """the slices are reused from render to render without any clearing: the second render of a frame
    from one context is the first, and so are its counters"""
    scene = two_run_scene(tmp_path, (1024, 65))
    r = rtxpy.Renderer(0)
    try:
        r.upload(scene)
        r.set_option(abi.RTX_OPT_SHADOW_SLOT, 64)
        r.set_option(abi.RTX_OPT_SHADOW_ORDER, 1)
        frames = []
        for count in (0, 0, 1, 1):
            p = bench_params(2, 3)
            p.count_traversal = count
            rgb, z = r.render(scene.frame(64, 36), p)
            frames.append((rgb.tobytes(), z.tobytes(), r.stats()))
    finally:
        r.close()
    for a, b in ((0, 1), (1, 2), (2, 3)):
        assert frames[a][0] == frames[b][0] and frames[a][1] == frames[b][1], (a, b)
    s2, s3 = frames[2][2], frames[3][2]
    assert s2.shadow_ordered_points > 0
    assert (s2.shadow_ordered_points, s2.shadow_ordered_rays, s2.shadow_wave_steps) == \
        (s3.shadow_ordered_points, s3.shadow_ordered_rays, s3.shadow_wave_steps)
