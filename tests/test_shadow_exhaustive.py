"""The CPU half of the exhaustive shadow-query check: the candidate filter of
rays_exhaustive.py loses no acceptance of the any-hit tests, every (ray, plane) pair is one float64
can decide, and the families are not vacuous (rays through a dozen transparent surfaces, blocked
and unblocked rays side by side, no far ray that needs the far-sphere exception)."""
import numpy as np
import pytest

import rays_exhaustive as RX
import shadow_exhaustive as SX
from rtxpy import abi, oracle

BRUTE = 256  # rays per family whose decisions are also taken over every bounded object
# the filter sees geometry only: glass has mixed's bounded objects, record for record
FILTER_SCENES = ("mixed", "trionly", "tiny")


class Cpu:
    def __init__(self, tmp):
        self.paths = SX.write_scenes(tmp)
        self.scenes, self.fams, self.mats, self.data = {}, {}, {}, {}

    def objs(self, key):
        if key not in self.scenes:
            self.scenes[key] = RX.load(self.paths[key])
            objs = RX.objects_of(self.scenes[key])
            self.mats[key] = SX.Mats(self.scenes[key], objs)
            self.fams[key] = SX.families(objs, key[1], key[0])
        return RX.objects_of(self.scenes[key])

    def get(self, key, fam):
        if (key, fam) not in self.data:
            objs = self.objs(key)
            rays = SX.mixed(self.fams[key])[0] if fam == "mixed" else self.fams[key][fam]
            self.data[key, fam] = SX.Data(objs, self.mats[key], rays, oracle.kat)
        return self.data[key, fam]

    def close(self):
        for s in self.scenes.values():
            s.close()


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    c = Cpu(tmp_path_factory.mktemp("shadow_exhaustive"))
    yield c
    c.close()


KEYS = [(s, v) for s in SX.SCENES for v in SX.VARIANTS]
ids = lambda keys: ["%s-%s" % k for k in keys]


@pytest.mark.parametrize("key", KEYS, ids=ids(KEYS))
def test_scene_records(cpu, key):
    objs = cpu.objs(key)
    mats = cpu.mats[key]
    bounded = objs["type"] != abi.RTX_PLANE
    assert int((objs["num_lights"] > 0).sum()) == 2 and not mats.transparent[objs["num_lights"] > 0].any()
    spheres = int(((objs["type"] == abi.RTX_SPHERE) & (objs["num_lights"] == 0)).sum())
    if key[0] == "tiny":
        assert bounded.sum() <= abi.RTX_SHADOW_LINEAR_MAX and spheres == 2
    else:
        assert bounded.sum() == 2112 + 5120 + 2 + spheres and spheres == (0 if key[0] == "trionly" else 1)
    if key[0] == "glass":
        assert mats.transparent[objs["num_lights"] == 0].all()
    else:
        assert mats.transparent[bounded].any() and not mats.transparent[bounded].all()
        planes = objs["type"] == abi.RTX_PLANE
        assert sorted(mats.channel[planes]) == [-1, 2]


FILTER_KEYS = [(s, v) for s in FILTER_SCENES for v in SX.VARIANTS]


@pytest.mark.parametrize("fam", SX.FAMILIES)
@pytest.mark.parametrize("key", FILTER_KEYS, ids=ids(FILTER_KEYS))
def test_filter_loses_no_acceptance(cpu, key, fam):
    objs = cpu.objs(key)
    D = cpu.get(key, fam)
    r = D.rays
    bounded = np.nonzero(objs["type"] != abi.RTX_PLANE)[0]
    rows = np.nonzero(~r.idle)[0][:BRUTE]
    pr, po = np.repeat(rows, len(bounded)), np.tile(bounded, len(rows))
    hit = RX.any_pairs(oracle.kat, objs, r.o, r.d, r.dist, pr, po)
    n = len(objs)
    accepted = set((pr[hit].astype(np.int64) * n + po[hit]).tolist())
    cand = set((D.P.pr.astype(np.int64) * n + D.P.po).tolist())
    print(key, fam, "candidates per ray", len(D.P.pr) / max(1, (~r.idle).sum()), "accepted", len(accepted), "lost", len(accepted - cand))
    assert accepted and not accepted - cand


@pytest.mark.parametrize("key", KEYS, ids=ids(KEYS))
def test_every_plane_pair_is_decisive(cpu, key):
    cpu.objs(key)
    pairs = 0
    for fam in SX.FAMILIES:
        P = SX.candidates(cpu.objs(key), cpu.fams[key][fam]) if (key[0] not in FILTER_SCENES) else cpu.get(key, fam).P
        pairs += P.plane_pairs
        assert P.plane_shaky == 0, (key, fam, P.plane_shaky)
    print(key, "plane pairs", pairs)


@pytest.mark.parametrize("key", [("glass", v) for v in SX.VARIANTS] + [("mixed", v) for v in SX.VARIANTS], ids=lambda k: "%s-%s" % k)
def test_through_rays_cross_a_dozen_transparent_surfaces(cpu, key):
    D = cpu.get(key, "through")
    hits = D.expo.sum(1)
    print(key, "through: transparent hits per ray, max", int(hits.max()), "rays with 12 or more", int((hits >= 12).sum()))
    assert (hits >= 12).sum() >= 256
    assert D.expo.max() <= SX.MAX_EXPONENT


@pytest.mark.parametrize("key", [(s, v) for s in ("mixed", "trionly") for v in SX.VARIANTS], ids=lambda k: "%s-%s" % k)
def test_mixed_batch_has_blocked_and_unblocked_rays(cpu, key):
    D = cpu.get(key, "mixed")
    share = float(D.blocked.mean())
    print(key, "mixed batch: blocked share", share, "max exponent", int(D.expo.max()))
    assert 0.1 <= share <= 0.9
    assert D.expo.max() <= SX.MAX_EXPONENT
    assert (D.tm[~D.blocked] != 1).any(1).mean() >= 0.1  # unblocked rays that crossed something transparent


@pytest.mark.parametrize("key", [(s, v) for s in ("glass", "mixed", "trionly") for v in SX.VARIANTS], ids=lambda k: "%s-%s" % k)
def test_far60_needs_no_far_sphere_exception(cpu, key):
    objs = cpu.objs(key)
    D = cpu.get(key, "far60")
    far = RX.far_mask(cpu.scenes[key], objs, D.rays.o)
    assert far.all()
    sph = D.P.sphere & D.hit
    print(key, "far60: sphere acceptances", int(sph.sum()), "exempt", D.exempt(far))
    assert D.exempt(far) == 0


@pytest.mark.parametrize("key", [("mixed", v) for v in SX.VARIANTS], ids=lambda k: "%s-%s" % k)
def test_light_family_targets_behind_the_emitter_are_blocked_without_the_skip(cpu, key):
    objs = cpu.objs(key)
    r = cpu.fams[key]["light"]
    assert r.target_far.sum() >= 64 and (r.light >= 0).all() and (objs["num_lights"][r.light] > 0).all()
    D = SX.Data(objs, cpu.mats[key], r.without_light(), oracle.kat, cpu.get(key, "light").P)
    assert D.blocked[r.target_far].all()
    assert (D.blocked != cpu.get(key, "light").blocked).sum() >= r.target_far.sum() // 2
