"""A numpy audit of the trees rtx_upload_scene builds: no GPU and no rtxpy calls, arrays in
and a report out.

Every walk culls with boxes, so every tree rests on one promise: each box on the path from the root to a
primitive contains that primitive, after the tree-frame rotation, the padding, the 16-bit quantisation and
the 8-bit outward rounding in the node's own frame.  The audits here check that promise, and the structure
around it, on the records rtx_read_wide_tree and rtx_read_bvh2 copy back (csrc/rtx_device.h: DW8, DNode,
DPrim, DQNode):

  audit_wide      the 8-wide compressed tree
  audit_bvh2      the float BVH2
  audit_threaded  the threaded 16-bit copy of the BVH2

A primitive's extent is formed in float64 from its float32 scene record (a triangle's vertices p0, p0 + e1,
p0 + e2, the points its intersector tests; a sphere's centre +- radius along each frame axis), mapped into
the trees' frame with x' = R (x - c) for the float32 R and c the kernels use, and, for the quantised trees,
onto their grid with g = (x' - qo) * qs.  Containment takes no tolerance: the slack must be >= 0.  Since a
box holds every primitive below it exactly when it holds their union, each audit carries the union of the
extents up the tree and compares it with every box on the way.

Each audit returns a Report: `violations`, a list of tuples whose first item names the kind, and
`figures`, what was measured on the way (depth, counts, the smallest slack and where it occurred).
"""
import sys

import numpy as np

SPHERE, TRIANGLE, PLANE = 0, 1, 2           # include/rtx.h enum rtx_object_type
REF_LEAF, REF_SPH, REF_CNT = 32, 16, 15     # csrc/rtx_device.h RTX_REF_*
EMPTY_REF = 0xFFFFFFFF
META_TRANSPARENT = 0x800000
MAX_EXPONENT = 9                            # rtx_device.h DW8: "a per-axis step of 2^e grid units (e <= 9)"
GRID_MAX = 65535


class Report:
    def __init__(self):
        self.violations = []
        self.figures = {}

    def add(self, *what):
        self.violations.append(tuple(what))

    def kinds(self):
        return sorted(set(v[0] for v in self.violations))


def scene_words(objs, transparent):
    """words 0..11 of the DPrim record (a, b, c) of every object of the scene records `objs`
    (rays_exhaustive.OBJ_DTYPE), as rtx_scene.cpp make_prim forms them; transparent: per object"""
    n = len(objs)
    w = np.zeros((n, 12), np.uint32)
    f = w.view(np.float32)
    tri, sph = objs["type"] == TRIANGLE, objs["type"] == SPHERE
    f[:, 0:3] = objs["p0"]
    f[:, 3] = objs["epsilon"]
    f[tri, 4:7] = objs["e1"][tri]
    f[sph, 4] = objs["radius"][sph]
    w[:, 7] = np.arange(n, dtype=np.uint32)
    f[tri, 8:11] = objs["e2"][tri]
    w[:, 11] = ((objs["type"].astype(np.uint32) << 24) | objs["material"].astype(np.uint32)
                | np.where(np.asarray(transparent, bool), META_TRANSPARENT, 0).astype(np.uint32))
    return w


def extents(objs, R, c):
    """(lo, hi), float64 (n, 3): every bounded object's extent in the frame x' = R (x - c); NaN rows for planes"""
    R, c = np.asarray(R, np.float32).astype(np.float64).reshape(3, 3), np.asarray(c, np.float32).astype(np.float64)
    n = len(objs)
    lo, hi = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    tri, sph = np.nonzero(objs["type"] == TRIANGLE)[0], np.nonzero(objs["type"] == SPHERE)[0]
    if len(tri):
        p0, e1, e2 = (objs[k][tri].astype(np.float64) for k in ("p0", "e1", "e2"))
        v = np.stack([p0, p0 + e1, p0 + e2])  # exact in float64
        x = (v - c) @ R.T
        lo[tri], hi[tri] = x.min(0), x.max(0)
    if len(sph):
        ctr = (objs["p0"][sph].astype(np.float64) - c) @ R.T
        r = np.abs(objs["radius"][sph].astype(np.float64))[:, None] * np.linalg.norm(R, axis=1)[None]
        lo[sph], hi[sph] = ctr - r, ctr + r
    return lo, hi


class _Slack:
    """the smallest containment slack seen and where"""

    def __init__(self):
        self.value, self.where = np.inf, None

    def see(self, slack_lo, slack_hi, **where):
        s = np.concatenate([slack_lo, slack_hi])
        k = int(np.argmin(s))
        if s[k] < self.value:
            self.value = float(s[k])
            self.where = dict(where, axis="xyz"[k % 3], side="lo" if k < 3 else "hi")


def _deep():
    if sys.getrecursionlimit() < 20000:
        sys.setrecursionlimit(20000)


# ---- the 8-wide tree ----
def audit_wide(entries, frame, objs, tree_R, tree_c, skip_objects, transparent=None, prims=None, stats=None):
    """entries: uint32 (n, 16), frame: its 16-bit frame (qo, qs), float32 (6,) (rtx_read_wide_tree); objs: the
    scene's records; tree_R, tree_c: the trees' frame; skip_objects: the objects the tree leaves out (the
    emitters).  transparent: per object, its material's flag (default: none is).  prims: the BVH2's primitive
    records (rtx_read_bvh2), to check the leaf entries' record indices against.  stats: wide_depth,
    wide_nodes and wide_entries to compare with (attributes or keys)."""
    rep = Report()
    ent = np.asarray(entries, np.uint32).reshape(-1, 16)
    n = len(ent)
    frame = np.asarray(frame, np.float32).astype(np.float64)
    qo, qs = frame[:3], frame[3:]
    transparent = np.zeros(len(objs), bool) if transparent is None else np.asarray(transparent, bool)
    words = scene_words(objs, transparent)
    lo, hi = extents(objs, tree_R, tree_c)
    glo, ghi = (lo - qo) * qs, (hi - qo) * qs
    bounded = objs["type"] != PLANE
    skip = set(int(x) for x in skip_objects)
    want = set(int(i) for i in np.nonzero(bounded)[0]) - skip
    seen_obj, seen_entry, seen_base = {}, set(), set()
    slack = _Slack()
    fig = dict(nodes=0, leaves=0, depth=0, max_exponent=0, clamped=0, boxes=0)
    if n < 2:
        rep.add("short tree", n)
        rep.figures = fig
        return rep
    if ent[1].any():
        rep.add("entry 1 is no hole", 1)

    def node(e, level):
        """audits node entry e; returns the union of its primitives' grid extents (lo, hi) and its depth"""
        w = ent[e]
        fig["nodes"] += 1
        org = np.array([w[0] & 0xFFFF, w[0] >> 16, w[1] & 0xFFFF], np.float64)
        ex = np.array([(w[1] >> 16) & 15, (w[1] >> 20) & 15, (w[1] >> 24) & 15], np.int64)
        if int(w[1]) >> 28:
            rep.add("header bits", e)
        base, imask = int(w[2]) >> 8, int(w[2]) & 0xFF
        vmask, tmask = int(w[3]) & 0xFF, (int(w[3]) >> 8) & 0xFF
        if int(w[3]) >> 16:
            rep.add("header bits", e)
        fig["max_exponent"] = max(fig["max_exponent"], int(ex.max()))
        if ex.max() > MAX_EXPONENT:
            rep.add("exponent", e, ex.tolist())
        if imask & ~vmask:
            rep.add("imask outside vmask", e, imask & ~vmask)
        if tmask & ~vmask or tmask & imask:
            rep.add("tmask", e, "on a slot that is no leaf", tmask & (~vmask | imask))
        planes = ent[e, 4:16].copy().view(np.uint8).reshape(3, 2, 8).astype(np.float64)  # [axis][lo, hi][slot]
        step = np.ldexp(1.0, ex)
        ulo, uhi = np.full(3, np.inf), np.full(3, -np.inf)
        depth = 1
        if not vmask:
            rep.add("empty node", e)
        if base < 2 or base + 8 > n:
            rep.add("block out of range", e, base)
            return ulo, uhi, depth
        if base in seen_base:
            rep.add("block shared", e, base)
            return ulo, uhi, depth
        seen_base.add(base)
        for s in range(8):
            if not (vmask >> s) & 1:
                if (planes[:, 0, s] != 255).any() or (planes[:, 1, s] != 0).any():
                    rep.add("empty slot not empty", e, s)
                continue
            child = base + s
            if child in seen_entry:
                rep.add("entry reached twice", child)
                continue
            seen_entry.add(child)
            blo, bhi = org + planes[:, 0, s] * step, org + planes[:, 1, s] * step
            fig["boxes"] += 1
            if (blo <= 0).any() or (bhi >= GRID_MAX).any():
                fig["clamped"] += 1
            if (imask >> s) & 1:
                clo, chi, d = node(child, level + 1)
                depth = max(depth, 1 + d)
            else:
                fig["leaves"] += 1
                lw = ent[child]
                obj = int(lw[7])
                if obj >= len(objs) or not bounded[obj]:
                    rep.add("leaf of no bounded object", child, obj)
                    continue
                if obj in seen_obj:
                    rep.add("object twice", obj, seen_obj[obj], child)
                seen_obj.setdefault(obj, child)
                if obj in skip:
                    rep.add("skipped object in the tree", obj, child)
                if not np.array_equal(lw[:12], words[obj]):
                    rep.add("leaf record", child, obj, [k for k in range(12) if lw[k] != words[obj][k]])
                if prims is not None and (int(lw[15]) >= len(prims) or int(prims[int(lw[15])][7]) != obj):
                    rep.add("leaf record index", child, obj, int(lw[15]))
                if bool((tmask >> s) & 1) != bool(int(lw[11]) & META_TRANSPARENT):
                    rep.add("tmask", e, s, obj)
                clo, chi = glo[obj], ghi[obj]
            if np.isfinite(clo).all():
                s_lo, s_hi = clo - blo, bhi - chi
                slack.see(s_lo, s_hi, entry=e, slot=s, level=level)
                if (s_lo < 0).any() or (s_hi < 0).any():
                    rep.add("containment", e, s, level, float(min(s_lo.min(), s_hi.min())))
                ulo, uhi = np.minimum(ulo, clo), np.maximum(uhi, chi)
        return ulo, uhi, depth

    _deep()
    seen_entry.add(0)
    _, _, fig["depth"] = node(0, 0)
    for obj in sorted(want - set(seen_obj)):
        rep.add("object missing", obj)
    fig["entries"] = n
    fig["min_slack"], fig["min_slack_at"] = slack.value, slack.where
    if stats is not None:
        get = (lambda k: stats[k]) if isinstance(stats, dict) else (lambda k: getattr(stats, k))
        for key, val in (("wide_depth", fig["depth"]), ("wide_nodes", fig["nodes"]), ("wide_entries", n)):
            if get(key) != val:
                rep.add("stats", key, get(key), val)
    rep.figures = fig
    return rep


# ---- the float BVH2 ----
def _leaf_range(ref, nnodes):
    return ((int(ref) & ~63) >> 6) - nnodes, (int(ref) & REF_CNT) + 1


def audit_bvh2(nodes, prims, root_ref, objs, R, c, max_leaf=16, transparent=None, depth=None):
    """nodes: uint32 (nnodes, 16) DNode records, prims: uint32 (nprims, 16) DPrim records in leaf order,
    root_ref (rtx_read_bvh2); objs: the scene's records; R, c: the trees' frame; max_leaf: RTX_OPT_BVH_LEAF;
    depth: stats.bvh_depth to compare with (inner nodes above the deepest leaf)"""
    rep = Report()
    nodes, prims = np.asarray(nodes, np.uint32).reshape(-1, 16), np.asarray(prims, np.uint32).reshape(-1, 16)
    boxes = nodes.view(np.float32).astype(np.float64)
    nn, nprim = len(nodes), len(prims)
    transparent = np.zeros(len(objs), bool) if transparent is None else np.asarray(transparent, bool)
    words = scene_words(objs, transparent)
    lo, hi = extents(objs, R, c)
    bounded = np.nonzero(objs["type"] != PLANE)[0]
    fig = dict(nodes=0, leaves=0, depth=0, prims=nprim)
    slack = _Slack()
    # the primitive records: every bounded object once, its record the scene's
    pobj = prims[:, 7].astype(np.int64)
    ok = pobj < len(objs)
    if not ok.all() or not np.array_equal(np.sort(pobj), bounded):
        rep.add("primitive records are not the bounded objects", nprim, len(bounded))
        pobj = np.where(ok, pobj, 0)
    bad = np.nonzero((prims[:, :12] != words[pobj]).any(1))[0]
    for k in bad[:8]:
        rep.add("primitive record", int(k), int(pobj[k]))
    tri = objs["type"][pobj] == TRIANGLE
    nrm = prims[:, 12:15].view(np.float32)
    badn = np.nonzero(tri & (nrm.view(np.uint32) != objs["n"][pobj].view(np.uint32)).any(1))[0]
    for k in badn[:8]:
        rep.add("primitive normal", int(k), int(pobj[k]))
    covered = np.zeros(nprim, np.int64)
    seen = np.zeros(nn, bool)

    def visit(ref, level):
        """returns the union of the extents below ref"""
        ref = int(ref)
        if ref & REF_LEAF:
            first, cnt = _leaf_range(ref, nn)
            fig["leaves"] += 1
            fig["depth"] = max(fig["depth"], level)
            if first < 0 or first + cnt > nprim:
                rep.add("leaf range", ref, first, cnt)
                return np.full(3, np.inf), np.full(3, -np.inf)
            if cnt > max_leaf:
                rep.add("leaf count", ref, cnt)
            covered[first:first + cnt] += 1
            o = pobj[first:first + cnt]
            if (objs["type"][o] == SPHERE).any() and not ref & REF_SPH:
                rep.add("sphere flag", ref)
            return lo[o].min(0), hi[o].max(0)
        i = ref >> 6
        if ref & 63 or i >= nn:
            rep.add("node ref", ref)
            return np.full(3, np.inf), np.full(3, -np.inf)
        if seen[i]:
            rep.add("node reached twice", i)
            return np.full(3, np.inf), np.full(3, -np.inf)
        seen[i] = True
        fig["nodes"] += 1
        ulo, uhi = np.full(3, np.inf), np.full(3, -np.inf)
        for k in range(2):
            clo, chi = visit(nodes[i, 12 + k], level + 1)
            b = boxes[i, 6 * k:6 * k + 6]
            if np.isfinite(clo).all():
                s_lo, s_hi = clo - b[0::2], b[1::2] - chi
                slack.see(s_lo, s_hi, node=i, child=k, level=level)
                if (s_lo < 0).any() or (s_hi < 0).any():
                    rep.add("containment", i, k, level, float(min(s_lo.min(), s_hi.min())))
                ulo, uhi = np.minimum(ulo, clo), np.maximum(uhi, chi)
        return ulo, uhi

    _deep()
    if int(root_ref) == EMPTY_REF:
        if nprim or nn:
            rep.add("empty root over records", nn, nprim)
    else:
        visit(root_ref, 0)
        if (covered != 1).any():
            rep.add("primitives not in exactly one leaf", np.nonzero(covered != 1)[0][:8].tolist())
        if fig["nodes"] != nn:
            rep.add("node count", nn, fig["nodes"])
    if depth is not None and depth != fig["depth"]:
        rep.add("stats", "bvh_depth", depth, fig["depth"])
    fig["min_slack"], fig["min_slack_at"] = slack.value, slack.where
    rep.figures = fig
    return rep


# ---- the threaded 16-bit copy ----
def audit_threaded(qnodes, frame, nnodes, prims, objs, R, c):
    """qnodes: uint32 (nq, 4) DQNode records in preorder, frame: their 16-bit frame (qo, qs) (rtx_read_bvh2);
    nnodes: the BVH2's inner-node count (leaf refs count records from it); prims: the BVH2's primitive records"""
    rep = Report()
    q = np.asarray(qnodes, np.uint32).reshape(-1, 4)
    prims = np.asarray(prims, np.uint32).reshape(-1, 16)
    nq, nprim = len(q), len(prims)
    frame = np.asarray(frame, np.float32).astype(np.float64)
    qo, qs = frame[:3], frame[3:]
    lo, hi = extents(objs, R, c)
    glo, ghi = (lo - qo) * qs, (hi - qo) * qs
    pobj = np.minimum(prims[:, 7].astype(np.int64), len(objs) - 1)
    covered = np.zeros(nprim, np.int64)
    slack = _Slack()
    fig = dict(qnodes=nq, leaves=0, depth=0, clamped=0)

    def parse(i, level):
        """the subtree at record i: (the index after it, the union of its extents)"""
        none = (np.full(3, np.inf), np.full(3, -np.inf))
        if i >= nq:
            rep.add("subtree runs past the end", i)
            return i, none[0], none[1]
        x = q[i]
        blo, bhi = (x[:3] & 0xFFFF).astype(np.float64), (x[:3] >> 16).astype(np.float64)
        if (blo <= 0).any() or (bhi >= GRID_MAX).any():
            fig["clamped"] += 1
        link = int(x[3])
        if link & REF_LEAF:
            fig["leaves"] += 1
            fig["depth"] = max(fig["depth"], level)
            first, cnt = _leaf_range(link, nnodes)
            end = i + 1
            if first < 0 or first + cnt > nprim:
                rep.add("leaf range", i, first, cnt)
                return end, none[0], none[1]
            covered[first:first + cnt] += 1
            o = pobj[first:first + cnt]
            ulo, uhi = glo[o].min(0), ghi[o].max(0)
        else:
            j, alo, ahi = parse(i + 1, level + 1)
            end, blo2, bhi2 = parse(j, level + 1)
            if link & 63 or link >> 6 != end:
                rep.add("link", i, link >> 6, end)
            ulo, uhi = np.minimum(alo, blo2), np.maximum(ahi, bhi2)
        if np.isfinite(ulo).all():
            s_lo, s_hi = ulo - blo, bhi - uhi
            slack.see(s_lo, s_hi, qnode=i, level=level)
            if (s_lo < 0).any() or (s_hi < 0).any():
                rep.add("containment", i, level, float(min(s_lo.min(), s_hi.min())))
        return end, ulo, uhi

    _deep()
    if nq:
        end, _, _ = parse(0, 0)
        if end != nq:
            rep.add("walk does not end at num_qnodes", end, nq)
        if (covered != 1).any():
            rep.add("leaf refs not visited exactly once", np.nonzero(covered != 1)[0][:8].tolist())
    elif nprim:
        rep.add("no threaded tree over primitives", nprim)
    fig["min_slack"], fig["min_slack_at"] = slack.value, slack.where
    rep.figures = fig
    return rep


# ---- two 8-wide trees against each other ----
def wide_tree_diff(ta, tb):
    """walk two 8-wide trees (rtx_read_wide_tree entries) from their roots in step and list where
    they differ: node words other than the child base (the layouts differ: host depth-first, device
    breadth-first), and the leaf entries (primitive record copies)"""
    names = ["w0 origin", "w1 origin/steps", "w2 inner mask", "w3 child/transparent masks"] + \
        [f"w{k} planes" for k in range(4, 16)]
    diffs = []
    q = [(0, 0, True)]
    while q:
        a, b, inner = q.pop()
        ea, eb = ta[a], tb[b]
        if not inner:  # leaf entries: the primitive record copies
            if not np.array_equal(ea, eb):
                diffs.append(("leaf", a, b, [k for k in range(16) if ea[k] != eb[k]]))
            continue
        wa, wb = ea.copy(), eb.copy()
        wa[2] &= 0xFF
        wb[2] &= 0xFF
        if not np.array_equal(wa, wb):
            diffs.append(("node", a, b, [names[k] for k in range(16) if wa[k] != wb[k]]))
            continue
        ba, bb = int(ea[2]) >> 8, int(eb[2]) >> 8
        for c in range(8):
            if (int(ea[3]) >> c) & 1:
                q.append((ba + c, bb + c, bool((int(ea[2]) >> c) & 1)))
    return diffs
