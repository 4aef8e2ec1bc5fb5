"""The conditions on the inputs of the hard-mesh tests (hard_meshes.py), on the CPU: the oracle's
float32 intersectors over every (ray, object) pair say that the ray families are not vacuous, so the GPU
tests cannot pass for want of hits."""
import numpy as np
import pytest

import hard_meshes as HM
import rays_exhaustive as RX
from rtxpy import abi, oracle


class Cpu:
    def __init__(self, tmp):
        self.paths = HM.write_scenes(tmp)
        self.scenes, self.res = {}, {}

    def get(self, name):
        """(scene, records, batch, rows of each family, brute force)"""
        if name not in self.res:
            scene = self.scenes[name] = HM.load(name, self.paths[name])
            objs = RX.objects_of(scene)
            rays, rows = HM.batch(HM.families(objs, name))
            self.res[name] = (scene, objs, rays, rows, HM.Brute(oracle.kat, scene, objs, rays))
        return self.res[name]

    def close(self):
        for s in self.scenes.values():
            s.close()


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    c = Cpu(tmp_path_factory.mktemp("hard_meshes"))
    yield c
    c.close()


BOUNDED = {"dupes": 600, "flat": 1152, "flat_rot": 1152, "slivers": 550, "scales": HM.SCALES_K * HM.SCALES_TRIS + 3, "offset": 320,
           "mixed": 342}
BOUNDED.update({"count%d" % n: n for n in HM.COUNTS})


@pytest.mark.parametrize("name", HM.SCENES)
def test_scene_is_what_the_catalogue_says(cpu, name):
    scene, objs, rays, rows, _ = cpu.get(name)
    assert int(HM.is_bounded(objs).sum()) == BOUNDED[name] <= 3000
    assert len(HM.emitters_of(scene)) == (2 if name == "mixed" else 0)
    assert rays.n == len(HM.FAMILIES) * HM.N_RAYS
    HM.assert_near(scene, objs, rays.o)
    HM.assert_near(scene, objs, rays.o, frame_world=True)
    if name == "dupes":
        assert len(np.unique(objs[["p0", "p1", "p2"]])) == 1
    if name in ("flat", "flat_rot"):
        lo, hi = RX.bounds(objs)
        assert ((hi - lo) == 0).sum() == (name == "flat")
    if name == "slivers":
        z = HM.zero_area(objs)
        assert z.sum() == 50 and (objs["p0"][z] == objs["p1"][z]).all(1).sum() == 5
    if name == "mixed":
        tr = HM.transparent_of(scene, objs)[HM.is_bounded(objs)]
        assert 0.3 <= tr.mean() <= 0.36
        assert (objs["type"] == abi.RTX_PLANE).sum() == 2 and (objs["type"] == abi.RTX_SPHERE).sum() == 41


@pytest.mark.parametrize("name", HM.SCENES)
def test_families_are_not_vacuous(cpu, name):
    scene, objs, rays, rows, B = cpu.get(name)
    hit = B.t > 0
    shares = {f: float(hit[rows[f]].mean()) for f in HM.FAMILIES}
    fams = HM.families(objs, name)
    print(name, "rays replaced as undecidable or too near a plane's thresholds", {f: fams[f].replaced for f in HM.FAMILIES})
    assert not HM.undecided(objs, rays.o, rays.d).any()
    print(name, "hit share", float(hit.mean()), shares, "blocked share", float(B.blocked.mean()), "max exponent", int(B.expo.max()))
    if name == "count0":
        assert set(objs["type"][B.po].tolist()) <= {abi.RTX_PLANE}
        return
    assert hit.mean() >= 0.25 and (~hit).mean() >= 0.10
    if name == "slivers":
        assert not HM.zero_area(objs)[B.po].any()
    if name == "scales":
        k = HM.scales_k(objs)
        obj = B.closest_objects()
        deep = (obj >= 0) & (k[np.maximum(obj, 0)] >= 12)
        print(name, "closest hits on k >= 12:", int(deep.sum()))
        assert deep.sum() >= 50
    if name == "mixed":
        assert B.expo.max() >= 2 and 0.05 <= B.blocked.mean() <= 0.95
