"""The audit of tree_audit.py can fail: a two-level 8-wide tree, a small BVH2 and its threaded copy are built
here in numpy (the two formulas of csrc/rtx_quant.h restated in a few lines), the audits report nothing on
them, and each fault planted in a copy is reported, alone.  No GPU."""
import numpy as np
import pytest

import rays_exhaustive as RX
import tree_audit as TA

F32, U32 = np.float32, np.uint32


# ---- rtx_quant.h, restated ----
def quantise(lo, hi, qo, qs):
    """rtx_quantise: (ql, qh) = floor((lo - qo) * qs) - 1, ceil((hi - qo) * qs) + 1, clamped to the 16-bit grid"""
    a = np.floor((np.float64(lo) - np.float64(qo)) * np.float64(qs)) - 1
    b = np.ceil((np.float64(hi) - np.float64(qo)) * np.float64(qs)) + 1
    return int(min(65535, max(0, a))), int(min(65535, max(0, b)))


def quantise8(ql, qh, org, e):
    """rtx_quantise8: the 16-bit pair relative to org in steps of 2^e, rounded outward"""
    return (ql - org) >> e, (qh - org + (1 << e) - 1) >> e


# ---- a small scene ----
N_TRI, N_SPH = 10, 3
EMITTER, PLANE_AT = 4, 7  # object 4 (a triangle) is the emitter the 8-wide tree leaves out; object 7 is a plane


def make_objs():
    rs = np.random.RandomState(7)
    objs = np.zeros(N_TRI + N_SPH + 1, RX.OBJ_DTYPE)
    kinds = [TA.TRIANGLE] * N_TRI + [TA.SPHERE] * N_SPH
    rs.shuffle(kinds)
    kinds.insert(PLANE_AT, TA.PLANE)
    kinds[EMITTER] = TA.TRIANGLE
    objs["type"] = kinds
    objs["material"] = rs.randint(0, 4, size=len(objs))
    objs["epsilon"] = 1e-4
    ctr = rs.uniform(-1, 1, size=(len(objs), 3)).astype(F32)
    objs["p0"] = ctr
    objs["e1"] = rs.uniform(-0.2, 0.2, size=(len(objs), 3)).astype(F32)
    objs["e2"] = rs.uniform(-0.2, 0.2, size=(len(objs), 3)).astype(F32)
    objs["radius"] = np.where(objs["type"] == TA.SPHERE, rs.uniform(0.05, 0.2, size=len(objs)), 0).astype(F32)
    objs["n"] = rs.normal(size=(len(objs), 3)).astype(F32)
    objs["num_lights"][EMITTER] = 4
    transparent = objs["material"] == 3
    assert transparent[objs["type"] != TA.PLANE].any() and not transparent.all()
    return objs, transparent


def float_boxes(objs):
    """every bounded object's float32 box, rounded outward from its float64 extent (world frame)"""
    lo, hi = TA.extents(objs, np.eye(3), np.zeros(3))
    lo32, hi32 = lo.astype(F32), hi.astype(F32)
    lo32 = np.where(lo32 > lo, np.nextafter(lo32, F32(-np.inf)), lo32)
    hi32 = np.where(hi32 < hi, np.nextafter(hi32, F32(np.inf)), hi32)
    return lo32, hi32


def frame_of(lo, hi):
    ext = hi - lo
    qs = (F32(65533) / np.maximum(ext, max(ext.max(), F32(1)) * F32(1e-6))).astype(F32)
    return np.concatenate([lo.astype(F32), qs])


def prim_records(objs, transparent, order):
    p = np.zeros((len(order), 16), U32)
    p[:, :12] = TA.scene_words(objs, transparent)[order]
    p[:, 12:15] = objs["n"][order].view(U32)
    return p


# ---- the 8-wide tree: a root with two inner children and two leaves, five leaves under each inner child ----
def make_wide(objs, transparent, lo32, hi32):
    inside = [i for i in np.nonzero(objs["type"] != TA.PLANE)[0] if i != EMITTER]
    assert len(inside) == 12
    groups = {"A": inside[0:5], "B": inside[5:10], "root": inside[10:12]}
    frame = frame_of(lo32[inside].min(0), hi32[inside].max(0))
    qo, qs = frame[:3], frame[3:]
    ent = np.zeros((2 + 3 * 8, 16), U32)
    words = TA.scene_words(objs, transparent)

    def node(me, base, kids):
        """kids: [(slot, lo, hi, inner, object)]"""
        q16 = [[quantise(lo[a], hi[a], qo[a], qs[a]) for a in range(3)] for _, lo, hi, _, _ in kids]
        org, ex = [], []
        for a in range(3):
            mn, mx = min(k[a][0] for k in q16), max(k[a][1] for k in q16)
            e = 0
            while ((mx - mn) + (1 << e) - 1) >> e > 255:
                e += 1
            org.append(mn)
            ex.append(e)
        planes = np.zeros((3, 2, 8), np.uint8)
        planes[:, 0, :] = 255
        imask = vmask = tmask = 0
        for (s, _, _, inner, obj), q in zip(kids, q16):
            for a in range(3):
                planes[a, 0, s], planes[a, 1, s] = quantise8(q[a][0], q[a][1], org[a], ex[a])
            vmask |= 1 << s
            if inner:
                imask |= 1 << s
            else:
                ent[base + s, :12] = words[obj]
                ent[base + s, 15] = obj  # (record index: the test's records are in object order)
                if transparent[obj]:
                    tmask |= 1 << s
        ent[me, 0] = org[0] | (org[1] << 16)
        ent[me, 1] = org[2] | (ex[0] << 16) | (ex[1] << 20) | (ex[2] << 24)
        ent[me, 2] = (base << 8) | imask
        ent[me, 3] = vmask | (tmask << 8)
        ent[me, 4:16] = planes.reshape(-1).view(U32)

    box = lambda g: (lo32[g].min(0), hi32[g].max(0))
    leafs = lambda g, slots: [(s, lo32[i], hi32[i], False, i) for s, i in zip(slots, g)]
    node(0, 2, [(0,) + box(groups["A"]) + (True, None), (3,) + box(groups["B"]) + (True, None)]
         + leafs(groups["root"], (5, 6)))
    node(2 + 0, 10, leafs(groups["A"], (1, 2, 4, 6, 7)))
    node(2 + 3, 18, leafs(groups["B"], (0, 1, 2, 3, 5)))
    return ent, frame, dict(wide_depth=2, wide_nodes=3, wide_entries=len(ent))


# ---- the BVH2 (median splits along x, leaves of at most two) and its threaded copy ----
def make_bvh2(objs, transparent, lo32, hi32):
    bounded = [int(i) for i in np.nonzero(objs["type"] != TA.PLANE)[0]]
    order, nodes = [], []

    deepest = [0]

    def build(ids, level=0):
        """returns (builder ref: ('leaf', first, cnt) or ('node', index), lo, hi)"""
        lo, hi = lo32[ids].min(0), hi32[ids].max(0)
        if len(ids) <= 2:
            deepest[0] = max(deepest[0], level)
            first = len(order)
            order.extend(ids)
            return ("leaf", first, len(ids)), lo, hi
        ids = sorted(ids, key=lambda i: lo32[i, 0] + hi32[i, 0])
        me = len(nodes)
        nodes.append(None)
        a, b = build(ids[:len(ids) // 2], level + 1), build(ids[len(ids) // 2:], level + 1)
        nodes[me] = (a, b)
        return ("node", me), lo, hi

    root, rlo, rhi = build(bounded)
    nn = len(nodes)

    def ref(r):
        if r[0] == "node":
            return r[1] * 64
        sph = TA.REF_SPH if (objs["type"][order[r[1]:r[1] + r[2]]] == TA.SPHERE).any() else 0
        return (nn + r[1]) * 64 | TA.REF_LEAF | sph | (r[2] - 1)

    rec = np.zeros((nn, 16), U32)
    f = rec.view(F32)
    for i, (a, b) in enumerate(nodes):
        for k, (r, lo, hi) in enumerate((a, b)):
            f[i, 6 * k + 0:6 * k + 6:2] = lo
            f[i, 6 * k + 1:6 * k + 6:2] = hi
            rec[i, 12 + k] = ref(r)
    prims = prim_records(objs, transparent, order)
    # the threaded copy: preorder, each node with the box it has in its parent (the scene bound for the root)
    frame = frame_of(rlo, rhi)
    q = []

    def thread(r, lo, hi):
        x = [quantise(lo[a], hi[a], frame[a], frame[3 + a]) for a in range(3)]
        me = len(q)
        q.append([x[0][0] | x[0][1] << 16, x[1][0] | x[1][1] << 16, x[2][0] | x[2][1] << 16, ref(r)])
        if r[0] == "node":
            for kr, klo, khi in nodes[r[1]]:
                thread(kr, klo, khi)
            q[me][3] = len(q) << 6

    thread(root, rlo, rhi)
    return rec, prims, ref(root), np.array(q, U32), frame, deepest[0]


@pytest.fixture(scope="module")
def trees():
    objs, transparent = make_objs()
    lo32, hi32 = float_boxes(objs)
    return dict(objs=objs, transparent=transparent, wide=make_wide(objs, transparent, lo32, hi32),
                bvh2=make_bvh2(objs, transparent, lo32, hi32))


I3, Z3 = np.eye(3, dtype=F32), np.zeros(3, F32)


def run_wide(t, ent, skip=(EMITTER,)):
    _, frame, stats = t["wide"]
    return TA.audit_wide(ent, frame, t["objs"], I3, Z3, skip, transparent=t["transparent"], stats=stats)


def run_bvh2(t, nodes=None, prims=None):
    rec, pr, root, _, _, depth = t["bvh2"]
    return TA.audit_bvh2(rec if nodes is None else nodes, pr if prims is None else prims, root, t["objs"], I3, Z3,
                         max_leaf=2, transparent=t["transparent"], depth=depth)


def run_threaded(t, q=None):
    rec, pr, _, qn, frame, _ = t["bvh2"]
    return TA.audit_threaded(qn if q is None else q, frame, len(rec), pr, t["objs"], I3, Z3)


def test_unplanted_trees_pass(trees):
    w, b, q = run_wide(trees, trees["wide"][0]), run_bvh2(trees), run_threaded(trees)
    assert not w.violations, w.violations
    assert not b.violations, b.violations
    assert not q.violations, q.violations
    assert w.figures["nodes"] == 3 and w.figures["leaves"] == 12 and w.figures["depth"] == 2
    assert 0 <= w.figures["min_slack"] < 4 * 2 ** w.figures["max_exponent"] and w.figures["max_exponent"] <= TA.MAX_EXPONENT
    assert b.figures["prims"] == 13 and b.figures["min_slack"] >= 0
    assert q.figures["qnodes"] == b.figures["nodes"] + b.figures["leaves"] and 0 <= q.figures["min_slack"] < 4


def planes(ent, e):
    """a view of node e's 8-bit planes, [axis][lo, hi][slot]"""
    return ent[e, 4:16].view(np.uint8).reshape(3, 2, 8)


def tightest(t, ent, e, slots, side):
    """(axis, slot) among node e's slots where raising lo8 / lowering hi8 by one must lose containment: the
    slack there is below one 8-bit step"""
    rep = run_wide(t, ent)
    assert not rep.violations
    _, frame, _ = t["wide"]
    qo, qs = frame[:3].astype(np.float64), frame[3:].astype(np.float64)
    lo, hi = TA.extents(t["objs"], I3, Z3)
    w = ent[e]
    org = [int(w[0]) & 0xFFFF, int(w[0]) >> 16, int(w[1]) & 0xFFFF]
    ex = [(int(w[1]) >> 16) & 15, (int(w[1]) >> 20) & 15, (int(w[1]) >> 24) & 15]
    base = int(w[2]) >> 8
    for s in slots:
        obj = int(ent[base + s, 7])
        for a in range(3):
            p = planes(ent, e)
            if side == 0 and (lo[obj, a] - qo[a]) * qs[a] < org[a] + (int(p[a, 0, s]) + 1) * 2 ** ex[a]:
                return a, s
            if side == 1 and (hi[obj, a] - qo[a]) * qs[a] > org[a] + (int(p[a, 1, s]) - 1) * 2 ** ex[a]:
                return a, s
    raise AssertionError("no tight plane")


def wide_fault(t, name):
    ent = t["wide"][0].copy()
    if name == "lo8 raised by one":
        a, s = tightest(t, ent, 2, (1, 2, 4, 6, 7), 0)
        planes(ent, 2)[a, 0, s] += 1
        return ent, "containment"
    if name == "hi8 lowered by one":
        a, s = tightest(t, ent, 5, (0, 1, 2, 3, 5), 1)
        planes(ent, 5)[a, 1, s] -= 1
        return ent, "containment"
    if name == "inner lo8 raised by one":  # the box of inner child A in the root: some primitive below it sticks out
        p = planes(ent, 0)
        for a in range(3):
            trial = ent.copy()
            planes(trial, 0)[a, 0, 0] += 1
            if run_wide(t, trial).violations:
                return trial, "containment"
        raise AssertionError("no tight plane")
    if name == "leaf dropped":
        ent[2, 3] &= ~U32(1 << 4 | 1 << (8 + 4))
        planes(ent, 2)[:, 0, 4], planes(ent, 2)[:, 1, 4] = 255, 0
        return ent, "object missing"
    if name == "leaf duplicated":  # node B's slot 2 again in its free slot 4, with the same planes
        ent[18 + 4] = ent[18 + 2]
        planes(ent, 5)[:, :, 4] = planes(ent, 5)[:, :, 2]
        tm = (int(ent[5, 3]) >> (8 + 2)) & 1
        ent[5, 3] |= U32(1 << 4 | tm << (8 + 4))
        return ent, "object twice"
    if name == "wrong tmask bit":
        ent[5, 3] ^= U32(1 << (8 + 3))
        return ent, "tmask"
    if name == "imask bit outside vmask":
        ent[2, 2] |= U32(1 << 0)
        return ent, "imask outside vmask"
    if name == "non-empty empty slot":
        planes(ent, 5)[1, 0, 7] = 3
        return ent, "empty slot not empty"
    if name == "exponent above 9":
        ent[2, 1] = (ent[2, 1] & ~U32(15 << 20)) | U32(10 << 20)
        planes(ent, 2)[1, 0, :] = np.where(planes(ent, 2)[1, 0, :] == 255, 255, 0)  # (keeps every box a container)
        return ent, "exponent"
    if name == "entry 1 written":
        ent[1, 5] = 1
        return ent, "entry 1 is no hole"
    if name == "block out of range":
        ent[5, 2] = U32(len(ent) - 4 << 8)
        return ent, None  # (its leaves go missing with it)
    if name == "block shared":
        ent[5, 2] = U32(10 << 8)
        return ent, None
    if name == "leaf record word":
        ent[10 + 6, 3] ^= U32(1)
        return ent, "leaf record"
    raise KeyError(name)


WIDE_FAULTS = ["lo8 raised by one", "hi8 lowered by one", "inner lo8 raised by one", "leaf dropped", "leaf duplicated",
               "wrong tmask bit", "imask bit outside vmask", "non-empty empty slot", "exponent above 9", "entry 1 written",
               "leaf record word"]


@pytest.mark.parametrize("name", WIDE_FAULTS)
def test_planted_wide_fault_is_reported_alone(trees, name):
    ent, kind = wide_fault(trees, name)
    rep = run_wide(trees, ent)
    assert rep.kinds() == [kind], (name, rep.violations)
    assert len(rep.violations) == 1, (name, rep.violations)


@pytest.mark.parametrize("name,kind", [("block out of range", "block out of range"), ("block shared", "block shared")])
def test_planted_block_fault_is_reported(trees, name, kind):
    ent, _ = wide_fault(trees, name)
    rep = run_wide(trees, ent)
    assert kind in rep.kinds() and set(rep.kinds()) <= {kind, "object missing", "stats"}, rep.violations


def test_wide_stats_and_skip_list_are_compared(trees):
    ent, frame, stats = trees["wide"]
    for key in stats:
        rep = TA.audit_wide(ent, frame, trees["objs"], I3, Z3, (EMITTER,), transparent=trees["transparent"],
                            stats=dict(stats, **{key: stats[key] + 1}))
        assert rep.violations == [("stats", key, stats[key] + 1, stats[key])]
    rep = run_wide(trees, ent, skip=())  # the emitter is expected in the tree, and is not there
    assert rep.violations == [("object missing", EMITTER)]
    inside = int(ent[10 + 1, 7])
    rep = run_wide(trees, ent, skip=(EMITTER, inside))
    assert rep.kinds() == ["skipped object in the tree"]


def test_planted_bvh2_faults_are_reported_alone(trees):
    rec, prims, root, _, _, depth = trees["bvh2"]
    base = run_bvh2(trees)
    at = base.figures["min_slack_at"]
    # the tightest float box, moved inward past the primitive
    bad = rec.copy()
    col = 6 * at["child"] + 2 * "xyz".index(at["axis"]) + (at["side"] == "hi")
    f = bad.view(F32)
    step = F32(2) * F32(abs(base.figures["min_slack"])) + F32(1e-6)
    f[at["node"], col] += step if at["side"] == "lo" else -step
    rep = run_bvh2(trees, nodes=bad)
    assert rep.kinds() == ["containment"], rep.violations
    # a leaf that takes one primitive more than its own: that one is then in two leaves, and the leaf holds three
    bad = rec.copy()
    leaf = [(i, k) for i in range(len(rec)) for k in (0, 1) if int(rec[i, 12 + k]) & TA.REF_LEAF
            and TA._leaf_range(rec[i, 12 + k], len(rec))[0] + 2 < len(prims) and int(rec[i, 12 + k]) & TA.REF_CNT == 1][0]
    bad[leaf[0], 12 + leaf[1]] += 1
    rep = run_bvh2(trees, nodes=bad)
    assert "primitives not in exactly one leaf" in rep.kinds() and "leaf count" in rep.kinds(), rep.violations
    # a primitive record of another object's words
    badp = prims.copy()
    badp[3, 0] ^= U32(1)
    assert run_bvh2(trees, prims=badp).kinds() == ["primitive record"]
    # the depth
    rep = TA.audit_bvh2(rec, prims, root, trees["objs"], I3, Z3, max_leaf=2, transparent=trees["transparent"], depth=depth + 1)
    assert rep.kinds() == ["stats"]
    # a sphere leaf without its flag
    bad = rec.copy()
    i, k = [(i, k) for i in range(len(rec)) for k in (0, 1) if int(rec[i, 12 + k]) & TA.REF_SPH][0]
    bad[i, 12 + k] &= ~U32(TA.REF_SPH)
    assert run_bvh2(trees, nodes=bad).kinds() == ["sphere flag"]


def test_planted_threaded_faults_are_reported_alone(trees):
    q = trees["bvh2"][3]
    inner = [i for i in range(len(q)) if not int(q[i, 3]) & TA.REF_LEAF]
    assert len(inner) >= 3
    for i in (inner[0], inner[1], inner[-1]):
        for d in (1, -1):  # a skip link off by one, either way
            bad = q.copy()
            bad[i, 3] = U32(((int(q[i, 3]) >> 6) + d) << 6)
            rep = run_threaded(trees, bad)
            assert rep.violations == [("link", i, (int(q[i, 3]) >> 6) + d, int(q[i, 3]) >> 6)], rep.violations
    # a 16-bit plane moved inward by two steps (the quantiser widened it by one)
    base = run_threaded(trees)
    at = base.figures["min_slack_at"]
    bad = q.copy()
    a = "xyz".index(at["axis"])
    bad[at["qnode"], a] = U32(int(q[at["qnode"], a]) + (2 if at["side"] == "lo" else -(2 << 16)))
    rep = run_threaded(trees, bad)
    assert rep.kinds() == ["containment"], rep.violations
    # a leaf dropped from the end
    rep = run_threaded(trees, q[:-1])
    assert "leaf refs not visited exactly once" in rep.kinds() or "subtree runs past the end" in rep.kinds()
