"""The definition of the closest-point queries (rtx_closest_point_object, csrc/rtx_nearest_math.h) against the
float64 model of nearest_model.py, on the hard meshes and both exhaustive scenes.  No device."""
import numpy as np
import pytest

import hard_meshes as HM
import nearest_model as NM
import rays_exhaustive as RX
import rtxpy
from rtxpy import abi

SCENES = tuple(HM.SCENES) + tuple(RX.ROTATION)


class Fixtures:
    def __init__(self, tmp):
        self.paths = NM.scene_paths(tmp)
        self.res = {}

    def get(self, name):
        """(scene, records, pair rows, pair points, host dist, host cp, model dist, model cp, ulp)"""
        if name not in self.res:
            path, load = self.paths[name]
            scene = load(path)
            objs = RX.objects_of(scene)
            idx, P = NM.pairs_of(objs)
            d32, cp32 = NM.host(objs, idx, P)
            d64, cp64 = NM.model(objs[idx], P)
            self.res[name] = (scene, objs, idx, P, d32, cp32, d64, cp64, NM.coord_ulp(objs[idx], P))
        return self.res[name]

    def close(self):
        for r in self.res.values():
            r[0].close()


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    f = Fixtures(tmp_path_factory.mktemp("nearest_model"))
    yield f
    f.close()


def test_fixtures_cover_every_object_type_and_the_degenerate_triangles(fx):
    seen, zero = set(), 0
    for name in SCENES:
        _, objs, idx, P, *_ = fx.get(name)
        seen |= set(objs["type"][idx].tolist())
        zero += int(HM.zero_area(objs)[idx].sum())
    assert seen == {abi.RTX_SPHERE, abi.RTX_TRIANGLE, abi.RTX_PLANE}
    assert zero >= 1000


@pytest.mark.parametrize("name", SCENES)
def test_dist_within_the_bound_of_float64(fx, name):
    _, objs, idx, P, d32, cp32, d64, cp64, ulp = fx.get(name)
    assert len(idx) or name == "count0"
    assert np.isfinite(d32).all() and np.isfinite(cp32).all() and (d32 >= 0).all(), name
    err = np.abs(d32.astype(np.float64) - d64) / ulp
    worst = float(err.max()) if len(err) else 0.0
    print("%s: %d pairs, worst dist error %.3f ulp of the coordinates" % (name, len(idx), worst))
    k = int(err.argmax()) if len(err) else 0
    assert worst <= NM.DIST_ULPS_BOUND, (name, worst, idx[k], P[k], d32[k], d64[k])
    # cp is the point dist is measured to: |P - cp| is dist, and cp is no nearer than the model's closest point
    back = np.sqrt(((P.astype(np.float64) - cp32) ** 2).sum(1))
    assert (np.abs(back - d32) <= NM.DIST_ULPS_BOUND * ulp).all(), name


def test_observed_error_is_the_recorded_one(fx):
    """the constant the bound is four times of is what these fixtures give on this host, rounded up"""
    worst = 0.0
    for name in SCENES:
        _, objs, idx, P, d32, cp32, d64, cp64, ulp = fx.get(name)
        if len(idx):
            worst = max(worst, float((np.abs(d32.astype(np.float64) - d64) / ulp).max()))
    print("worst dist error over every fixture: %.3f ulp" % worst)
    assert worst <= NM.DIST_ULPS_OBSERVED < 2 * worst + 1


def test_zero_area_triangles_answer_as_their_segment(fx):
    n = 0
    for name in SCENES:
        _, objs, idx, P, d32, cp32, d64, cp64, ulp = fx.get(name)
        z = np.nonzero(HM.zero_area(objs)[idx])[0]
        if not len(z):
            continue
        n += len(z)
        o = objs[idx[z]]
        seg = NM.segment_distance(o, P[z])
        assert (np.abs(d32[z] - seg) <= NM.DIST_ULPS_BOUND * ulp[z]).all(), name
        assert (NM.segment_distance(o, cp32[z]) <= NM.DIST_ULPS_BOUND * ulp[z]).all(), name
    assert n >= 1000


def test_named_cases():
    o = np.zeros(3, RX.OBJ_DTYPE)
    o["type"] = [abi.RTX_SPHERE, abi.RTX_PLANE, abi.RTX_TRIANGLE]
    o["p0"][0], o["radius"][0] = [1.0, 2.0, 3.0], 0.5
    o["n"][1], o["d"][1] = [0.0, 1.0, 0.0], -1.5
    o["p0"][2], o["e1"][2], o["e2"][2] = [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]
    d, cp = NM.host(o, [0, 0, 1, 2, 2, 2], [[1, 2, 3], [1, 2, 5], [4, 2, 7], [0.25, 0.25, -2], [-1, -1, 0], [2, 0.5, 0]])
    assert d.tolist() == [0.5, 1.5, 3.5, 2.0, np.float32(2 ** 0.5), np.float32(1.25 ** 0.5)]
    assert cp.tolist() == [[1.5, 2, 3], [1, 2, 3.5], [4, -1.5, 7], [0.25, 0.25, 0], [0, 0, 0], [1, 0, 0]]
    # a point, and a triangle of three equal vertices far from the origin
    o["p0"][2], o["e1"][2], o["e2"][2] = [1e4, -1e4, 1e4], 0, 0
    d, cp = NM.host(o, [2], [[1e4, -1e4 + 3, 1e4 + 4]])
    assert d.tolist() == [5.0] and cp.tolist() == [[1e4, -1e4, 1e4]]


def test_python_entry_is_the_c_entry(fx):
    scene, objs, idx, P, d32, cp32, *_ = fx.get("mixed")
    for k in range(0, len(idx), max(1, len(idx) // 50)):
        d, cp = rtxpy.closest_point_object(scene, int(idx[k]), P[k])
        assert d.view(np.uint32) == d32[k].view(np.uint32) and (cp.view(np.uint32) == cp32[k].view(np.uint32)).all()
    with pytest.raises(IndexError):
        rtxpy.closest_point_object(scene, scene.desc.num_objects, P[0])
