"""The CPU half of the exhaustive ray-query check (DESIGN §7.3 "Exhaustive check"): the candidate
filter of rays_exhaustive.py loses no float32 hit, the ray families are not vacuous, and the
oracle's float32 intersectors (the device's arithmetic, test_gpu_rays_exhaustive.py) agree with a
plain float64 restatement on every ray where float64 can decide."""
import numpy as np
import pytest

import rays_exhaustive as RX
from rtxpy import oracle

SCENES = ("world", "rotated")
BRUTE = 256  # rays per family whose float32 minimum is also taken over every object


class Cpu:
    def __init__(self, tmp):
        self.paths = RX.write_scenes(tmp)
        self.scenes, self.fams, self.res = {}, {}, {}

    def objs(self, name):
        if name not in self.scenes:
            self.scenes[name] = RX.load(self.paths[name])
            self.fams[name] = RX.families(RX.objects_of(self.scenes[name]), name)
        return RX.objects_of(self.scenes[name])

    def get(self, name, fam):
        """(o, d, float64 reference, float32 minimum over the candidates, the pairs' kat results)"""
        if (name, fam) not in self.res:
            objs = self.objs(name)
            o, d = self.fams[name][fam]
            ref = RX.reference(objs, o, d)
            hit, t = RX.kat_pairs(oracle.kat, objs, o, d, ref.cand_ray, ref.cand_obj)
            self.res[name, fam] = (o, d, ref, RX.ray_min(len(o), ref.cand_ray, hit, t), hit, t)
        return self.res[name, fam]

    def close(self):
        for s in self.scenes.values():
            s.close()


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    c = Cpu(tmp_path_factory.mktemp("rays_exhaustive"))
    yield c
    c.close()


@pytest.mark.parametrize("name", SCENES)
def test_scene_records(cpu, name):
    objs = cpu.objs(name)
    assert len(objs) == RX.N_OBJECTS
    assert int((objs["num_lights"] > 0).sum()) == 1


@pytest.mark.parametrize("fam", RX.FAMILIES)
@pytest.mark.parametrize("name", SCENES)
def test_filter_loses_nothing(cpu, name, fam):
    objs = cpu.objs(name)
    o, d, ref, tmin, _, _ = cpu.get(name, fam)
    pr, po = RX.all_pairs(BRUTE, len(objs))
    hit, t = RX.kat_pairs(oracle.kat, objs, o, d, pr, po)
    brute = RX.ray_min(BRUTE, pr, hit, t)
    lost = int((brute.view(np.uint32) != tmin[:BRUTE].view(np.uint32)).sum())
    print(name, fam, "candidates per ray", len(ref.cand_ray) / len(o), "lost", lost)
    assert lost == 0


FLOOR = {"incoherent": 0.95, "surface": 0.95, "axis": 0.95, "onezero": 0.95, "edges": 0.6, "far60": 0.6}


@pytest.mark.parametrize("fam", RX.FAMILIES)
@pytest.mark.parametrize("name", SCENES)
def test_families_are_not_vacuous(cpu, name, fam):
    _, _, ref, tmin, _, _ = cpu.get(name, fam)
    hit_share, decisive = float((tmin > 0).mean()), float(ref.decisive.mean())
    print(name, fam, "hit share", hit_share, "decisive share", decisive)
    assert 0.3 <= hit_share <= 1.0
    assert set(FLOOR) == set(RX.FLOORED)
    if fam in FLOOR:
        assert decisive >= FLOOR[fam]


@pytest.mark.parametrize("name", SCENES)
def test_float32_against_float64_on_decisive_rays(cpu, name):
    """the oracle's float32 intersectors against the float64 restatement: RX.T64_MEASURED holds the
    largest relative t differences seen here (both scenes; the near families and far60 apart),
    RX.T64_BOUND four times them, capped at the suite's 1e-4"""
    objs = cpu.objs(name)
    worst = {"near": 0.0, "far60": 0.0}
    for fam in RX.FLOORED:
        _, _, ref, tmin, hit, t = cpu.get(name, fam)
        hm, om, rel = RX.compare_with_float64(len(objs), ref, ref.cand_ray, ref.cand_obj, hit, t, tmin)
        print(name, fam, "decisive", int(ref.decisive.sum()), "hit/miss differs", hm, "object differs", om, "max rel", rel)
        assert hm == 0 and om == 0
        worst[RX.t64_class(fam)] = max(worst[RX.t64_class(fam)], rel)
    print(name, "largest relative t differences", worst)
    for k in worst:
        assert RX.T64_BOUND[k] == min(4 * RX.T64_MEASURED[k], 1e-4)
        assert worst[k] <= RX.T64_MEASURED[k] <= RX.T64_BOUND[k]
