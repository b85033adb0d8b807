"""The specification of the BVH builder (gravit_amd/csrc/lbvh.hip) in plain numpy, and a validator for the trees it emits.

reference_tree() predicts the BINARY tree of a build bit for bit: scene box and pad, Morton keys (Python integers), the stable sort, Karras' 2012
topology with the kernel's tie-break, the compaction of the live nodes and the 64-byte node and slot records.  It is written from the kernels as the
definition -- float32 where they use float32, in their operation order (the library is compiled without contraction, min / max are exact) -- but
top-down with an explicit stack where the kernel searches per node, and with the boxes as plain reductions over each child's slot range where the
kernel uses a base-32 table or a walk in LDS.

validate() checks a tree by its defining properties, whoever built it: the binary tree's shape, the slots against the mesh, every binary child box
against the triangles of its range, and the quantised 4-wide layout (walked in tandem with the collapse rule, since the device numbers a level's nodes in
block-arrival order) for containment and tightness in float64 and against the triangles directly.

Any change to the builder's key width, tie-break, pad or compaction order must change this file in the same commit.

Not modelled: the order of min / max over zeros of different sign (the cases keep away from -0.0), NaN coordinates, and extents that overflow float32."""
from collections import namedtuple

import numpy as np

F = np.float32
FLT_MAX = F(3.4028234663852886e38)
EMPTY_REF = -1
LEAF_MAX_LIMIT = 4
NB_CHUNK = 1024  # k_node_boxes_chunk's chunk of sorted triangles
CHUNKED_FROM = 4 * NB_CHUNK  # first triangle count whose node boxes are built per chunk in LDS
PACKET_SAH_MAX = 128  # the library's default for the knob packet_sah_max

Finding = namedtuple("Finding", "rule node slot detail")
MAX_PER_RULE = 8  # findings reported per rule (a broken tree breaks a rule thousands of times)


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=F)
    return a if shape is None else a.reshape(shape)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def key_bits(n):
    """build_lbvh: 18 bits, 3 more for every shift of n by 3 until it reaches 1, clamped to [30, 63] -- 30 up to 8,191 triangles, 33 from 8,192."""
    b, k = 18, int(n)
    while k > 1:
        b += 3
        k >>= 3
    return min(max(b, 30), 63)


def table_levels(n):
    """build_box_levels: levels of the base-32 range-union table over n sorted triangle boxes (level 0 = the boxes themselves)."""
    lv, cnt = 1, int(n)
    while cnt > 32 and lv < 6:
        cnt = (cnt + 31) // 32
        lv += 1
    return lv


def leaf_ref(first, count):
    return ~((int(first) << 3) | int(count))


def tri_boxes(verts, tris):
    p = _f32(verts, (-1, 3))[np.asarray(tris, np.int64).reshape(-1, 3)]  # (n, 3 corners, 3 axes)
    return p.min(1), p.max(1)


def scene_record(tlo, thi):
    """k_scene_box: (lo, hi, iso, pad) of the triangle boxes, all float32."""
    lo, hi = tlo.min(0), thi.max(0)
    ext = F(max(np.abs(lo).max(), np.abs(hi).max()))
    with np.errstate(all="ignore"):
        em = F(max(hi - lo))
        iso = F(1) / em if em > 0 else F(0)
        pad = ext * F(1e-5)
    return lo, hi, iso, pad


def _expand21(v):
    x = v & np.uint64(0x1FFFFF)
    for sh, mask in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(sh))) & np.uint64(mask)
    return x


def morton_keys(tlo, thi, lo, iso, bits):
    """k_morton: a list of Python integers, one key per triangle in input order."""
    with np.errstate(all="ignore"):
        c = (F(0.5) * (tlo + thi) - lo) * iso
        q = np.fmin(np.fmax(c * F(2097152.0), F(0)), F(2097151.0))
    q = q.astype(np.uint64)
    code = (_expand21(q[:, 0]) << np.uint64(2)) | (_expand21(q[:, 1]) << np.uint64(1)) | _expand21(q[:, 2])
    return [int(k) >> (63 - bits) for k in code.tolist()]


def delta(keys, i, j):
    """Common-prefix length of the strings (key, position) at sorted positions i and j (the kernel's delta; the caller keeps j inside the array)."""
    a, b = keys[i], keys[j]
    if a == b:
        return 64 + 32 - (i ^ j).bit_length()
    return 64 - (a ^ b).bit_length()


class Topology:
    """Slot order and Karras' tree over it: node i covers sorted positions first[i] .. last[i] and splits behind gamma[i]."""

    def __init__(self, n, leaf_max):
        self.n, self.leaf_max, self.single = n, leaf_max, n <= leaf_max
        self.key_bits = key_bits(n)
        self.keys = None  # sorted keys (Python integers)
        self.order = np.arange(n, dtype=np.int64)
        self.first = self.last = self.gamma = np.zeros(0, np.int64)


def karras_topology(verts, tris, leaf_max):
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    n = len(tris)
    T = Topology(n, leaf_max)
    if T.single:
        return T
    tlo, thi = tri_boxes(verts, tris)
    lo, _, iso, _ = scene_record(tlo, thi)
    keys = morton_keys(tlo, thi, lo, iso, T.key_bits)
    T.order = np.argsort(np.array(keys, dtype=np.uint64), kind="stable").astype(np.int64)
    K = T.keys = [keys[p] for p in T.order.tolist()]
    first, last, gamma = [0] * (n - 1), [0] * (n - 1), [0] * (n - 1)
    stack = [(0, 0, n - 1)]  # (node, first, last): the root is node 0
    while stack:
        i, f, l = stack.pop()
        dn = delta(K, f, l)
        a, b = f, l - 1  # the last position that shares more than the node's prefix with `first`
        while a < b:
            mid = (a + b + 1) >> 1
            if delta(K, f, mid) > dn:
                a = mid
            else:
                b = mid - 1
        first[i], last[i], gamma[i] = f, l, a
        if a > f:
            stack.append((a, f, a))  # the left inner child is node gamma (the last position of its range)
        if a + 1 < l:
            stack.append((a + 1, a + 1, l))  # the right one gamma + 1 (the first of its range)
    T.first, T.last, T.gamma = (np.array(x, np.int64) for x in (first, last, gamma))
    return T


def _range_reduce(ufunc, a, f, e):
    """ufunc-reduction of rows a[f[k]:e[k]] for every k (f < e <= len(a))."""
    a2 = np.concatenate([a, a[-1:]])
    idx = np.stack([np.asarray(f, np.int64), np.asarray(e, np.int64)], 1).ravel()
    return ufunc.reduceat(a2, idx, axis=0)[::2]


def slot_records(verts, tris, order):
    """k_emit_tris: (n, 16) float32 -- v0 | primID bits, e1 = v0 - v1 | v1.x, e2 = v2 - v0 | v1.y, v1.z, v2.xyz."""
    verts = _f32(verts, (-1, 3))
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    order = np.asarray(order, np.int64)
    p = verts[tris[order]]
    v0, v1, v2 = p[:, 0], p[:, 1], p[:, 2]
    out = np.zeros((len(order), 16), F)
    with np.errstate(all="ignore"):
        out[:, 0:3], out[:, 4:7], out[:, 8:11] = v0, v0 - v1, v2 - v0
    out.view(np.int32)[:, 3] = order.astype(np.int32)
    out[:, 7], out[:, 11], out[:, 12], out[:, 13:16] = v1[:, 0], v1[:, 1], v1[:, 2], v2
    return out


def _child_planes(nodes):
    """(n_nodes, 2 sides, 3 axes) lo and hi planes of the child boxes of binary nodes."""
    return nodes[:, [[0, 2, 8], [4, 6, 10]]], nodes[:, [[1, 3, 9], [5, 7, 11]]]


def child_areas(nodes):
    """slot_area of both children of every binary node: float32, summed left to right."""
    lo, hi = _child_planes(_f32(nodes))
    with np.errstate(all="ignore"):
        d = hi - lo
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        return dx * dy + dy * dz + dz * dx


def sah_inner(nodes, lo, hi):
    """build_lbvh / k_sah_sum: 1 + the 16.16 fixed-point sum over the nodes of the areas of their inner children, relative to the scene box's."""
    nodes = _f32(nodes)
    if len(nodes) <= 1:
        return F(0), 0
    refs = nodes.view(np.int32)[:, 12:14]
    with np.errstate(all="ignore"):
        ex, ey, ez = (F(hi[k]) - F(lo[k]) for k in range(3))
        ra = ex * ey + ey * ez + ez * ex
        total = 0
        if ra > 0:
            a = child_areas(nodes)
            s = np.where(refs[:, 0] >= 0, a[:, 0], F(0)) + np.where(refs[:, 1] >= 0, a[:, 1], F(0))
            v = np.fmin(s * (F(1) / ra), F(4)) * F(65536.0)
            total = sum(int(x) for x in v.tolist())
        out = F(1) + F(total / 65536.0)
    return out, int(out <= F(PACKET_SAH_MAX))


class Tree:
    pass


def reference_tree(verts, tris, leaf_max, topology=None):
    """The build of (verts, tris) under the knob leaf_max.  topology: a karras_topology() of EARLIER vertices -- the tree a refit keeps while the
    boxes, the pad and the slots follow the new ones."""
    verts = _f32(verts, (-1, 3))
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    n = len(tris)
    assert n >= 1 and 1 <= leaf_max <= LEAF_MAX_LIMIT
    T = topology if topology is not None else karras_topology(verts, tris, leaf_max)
    assert T.n == n and T.leaf_max == leaf_max
    R = Tree()
    R.topology, R.order, R.key_bits = T, T.order, T.key_bits
    tlo, thi = tri_boxes(verts, tris)
    R.bbox_lo, R.bbox_hi, R.iso, R.pad = scene_record(tlo, thi)
    pad = R.pad
    R.slots = slot_records(verts, tris, T.order)
    slo, shi = tlo[T.order], thi[T.order]
    with np.errstate(all="ignore"):
        if T.single:
            lo, hi = slo.min(0) - pad, shi.max(0) + pad
            nd = np.zeros((1, 16), F)
            nd[0, 0:4] = lo[0], hi[0], lo[1], hi[1]
            nd[0, 4:8] = FLT_MAX, -FLT_MAX, FLT_MAX, -FLT_MAX
            nd[0, 8:12] = lo[2], hi[2], FLT_MAX, -FLT_MAX
            nd.view(np.int32)[0, 12:14] = leaf_ref(0, n), EMPTY_REF
            R.nodes, R.n_nodes, R.n_leaves = nd, 1, 1
        else:
            first, last, gamma = T.first, T.last, T.gamma
            live = (last - first + 1) > leaf_max
            newidx = np.cumsum(live) - live  # exclusive prefix sum over i = 0 .. n-2
            i = np.nonzero(live)[0]
            nd = np.zeros((len(i), 16), F)
            ref = nd.view(np.int32)
            for side, (f, l, c) in enumerate(((first[i], gamma[i], gamma[i]), (gamma[i] + 1, last[i], gamma[i] + 1))):
                lo = _range_reduce(np.minimum, slo, f, l + 1) - pad
                hi = _range_reduce(np.maximum, shi, f, l + 1) + pad
                cnt = l - f + 1
                nd[:, 4 * side + 0], nd[:, 4 * side + 1], nd[:, 4 * side + 2], nd[:, 4 * side + 3] = lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1]
                nd[:, 8 + 2 * side], nd[:, 9 + 2 * side] = lo[:, 2], hi[:, 2]
                inner = newidx[np.minimum(c, n - 2)]  # (c is an inner node's number only where cnt > leaf_max)
                ref[:, 12 + side] = np.where(cnt <= leaf_max, ~((f << 3) | cnt), inner).astype(np.int32)
            out = np.zeros_like(nd)
            out[newidx[i]] = nd
            R.nodes, R.n_nodes = out, len(i)
            R.n_leaves = R.n_nodes + 1
    R.sah_inner, R.packet = sah_inner(R.nodes, R.bbox_lo, R.bbox_hi)
    return R


# ------------------------------------------------------------------------------------------------ the 4-wide collapse rule
def collapse_children(b, refs, areas):
    """k_collapse4's rule at binary node b: [(binary node, side)] of the up to four children, in slot order.  refs, areas: per-node [c0, c1] lists."""
    c = [(b, 0), (b, 1)]
    if refs[b][1] == EMPTY_REF:
        c = [(b, 0)]  # the single-leaf mesh
    for _ in range(2):
        if len(c) >= 4:
            break
        k, best = -1, -1.0
        for s, (nb, sd) in enumerate(c):
            if refs[nb][sd] >= 0 and areas[nb][sd] > best:  # strict: the lowest slot wins ties (and a NaN area never wins)
                best, k = areas[nb][sd], s
        if k < 0:
            break
        r = refs[c[k][0]][c[k][1]]
        c[k] = (r, 0)  # the left child into the replaced slot, the right one into the first free slot
        c.append((r, 1))
    return c


def decode4(nodes4):
    """origin (m, 3) float32, step words (m, 3) uint32, qlo / qhi (m, 4 children, 3 axes) int64, refs (m, 4) int32."""
    w = np.ascontiguousarray(nodes4, dtype=np.uint32).reshape(-1, 16)
    origin = w[:, 0:3].copy().view(F)
    step = w[:, [3, 14, 15]]
    sh = (8 * np.arange(4, dtype=np.uint32))[None, :, None]
    qlo = ((w[:, None, [4, 6, 8]] >> sh) & np.uint32(255)).astype(np.int64)
    qhi = ((w[:, None, [5, 7, 9]] >> sh) & np.uint32(255)).astype(np.int64)
    return origin, step, qlo, qhi, w[:, 10:14].copy().view(np.int32)


# ------------------------------------------------------------------------------------------------ the validator
class _Out(list):
    def add(self, rule, node, slot, detail):
        if sum(1 for f in self if f.rule == rule) < MAX_PER_RULE:
            self.append(Finding(rule, int(node), int(slot), detail))

    def add_where(self, rule, bad, node_of, detail):
        for k, s in zip(*np.nonzero(bad)[:2]):
            self.add(rule, node_of[k], s, detail)


def validate(verts, tris, nodes, nodes4, slots, leaf_max, collapse_from=None):
    """Findings (rule, node, slot, detail) of a tree over (verts, tris); an empty list: the tree is valid.  `slot` is the child slot of the node, or the
    triangle slot for the rules on slots.  nodes4 = None: the binary tree and the slots only.  collapse_from: the binary nodes whose areas chose the
    4-wide children -- after a refit those of the BUILD, since a refit keeps the 4-wide topology while `nodes` carry the new boxes."""
    out = _Out()
    verts = _f32(verts, (-1, 3))
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    n = len(tris)
    nodes = _f32(nodes).reshape(-1, 16)
    slots = _f32(slots).reshape(-1, 16)
    nn = len(nodes)
    refs = nodes.view(np.int32)[:, 12:14].tolist()

    # ---- the slots against the mesh
    prim = slots.view(np.int32)[:, 3].astype(np.int64)
    if len(slots) != n:
        out.add("slots.permutation", -1, len(slots), "%d slots for %d triangles" % (len(slots), n))
        return out
    cnt = np.bincount(np.clip(prim, 0, n - 1), minlength=n)
    if ((prim < 0) | (prim >= n)).any() or (cnt != 1).any():
        s = int(np.nonzero((prim < 0) | (prim >= n) | (cnt[np.clip(prim, 0, n - 1)] != 1))[0][0])
        out.add("slots.permutation", -1, s, "the primIDs are no permutation of 0..%d (slot %d holds %d)" % (n - 1, s, prim[s]))
    prim = np.clip(prim, 0, n - 1)
    want = slot_records(verts, tris, prim)
    want.view(np.int32)[:, 3] = slots.view(np.int32)[:, 3]
    for s in np.nonzero((_bits(want) != _bits(slots)).any(1))[0]:
        out.add("slots.geometry", -1, s, "the slot's floats are not those of triangle %d" % prim[s])

    # ---- the binary tree: reached once, leaves tile [0, n)
    single = nn == 1 and refs[0][1] == EMPTY_REF
    seen = [0] * nn
    order, leaves = [], []  # nodes in preorder; leaves (node, side, first, count) left to right
    stack = [(0, -1, 0)] if nn else []
    while stack:
        b, parent, side = stack.pop()
        if not 0 <= b < nn:
            out.add("binary.reach", parent, side, "reference %d outside the %d nodes" % (b, nn))
            continue
        seen[b] += 1
        if seen[b] > 1:
            out.add("binary.reach", parent, side, "node %d reached %d times" % (b, seen[b]))
            continue
        order.append(b)
        for sd in (1, 0):
            r = refs[b][sd]
            if r >= 0:
                stack.append((r, b, sd))
        # (a stack pops child 0's subtree first: leaves are collected in a second pass, in order)
    for b in range(nn):
        if seen[b] == 0:
            out.add("binary.reach", b, -1, "node %d not reached from the root" % b)
    if any(f.rule == "binary.reach" for f in out) or not nn:
        return out
    rng = [None] * nn  # slot range [first, end) of every node: child 0's start, child 1's end
    child_rng = np.zeros((nn, 2, 2), np.int64)
    for b in reversed(order):  # children come behind their parent in preorder
        for sd in (0, 1):
            r = refs[b][sd]
            if r >= 0:
                child_rng[b, sd] = rng[r]
            else:
                code = ~r
                child_rng[b, sd] = (code >> 3, (code >> 3) + (code & 7))
        rng[b] = (child_rng[b, 0, 0], child_rng[b, 1, 1])
    stack = [(0, 1), (0, 0)]
    while stack:
        b, sd = stack.pop()
        r = refs[b][sd]
        if r >= 0:
            stack.append((r, 1))
            stack.append((r, 0))
        elif not (single and sd == 1):
            leaves.append((b, sd, (~r) >> 3, (~r) & 7))
    if len(leaves) != (1 if single else nn + 1):
        out.add("binary.leaf_count", -1, -1, "%d leaves under %d nodes" % (len(leaves), nn))
    cursor = 0
    for b, sd, f, c in leaves:
        if not 1 <= c <= leaf_max:
            out.add("binary.leaf_size", b, sd, "a leaf of %d triangles (leaf_max %d)" % (c, leaf_max))
        if f != cursor:
            out.add("binary.tiling", b, sd, "the leaf starts at slot %d, the one before it ends at %d" % (f, cursor))
        cursor = f + c
    if cursor != n:
        out.add("binary.tiling", -1, -1, "the leaves end at slot %d of %d" % (cursor, n))

    # ---- every binary child box = the float32 union of the triangles of its range, padded in one operation
    tlo, thi = tri_boxes(verts, tris)
    _, _, _, pad = scene_record(tlo, thi)
    slo, shi = tlo[prim], thi[prim]
    blo, bhi = _child_planes(nodes)
    f, e = child_rng[..., 0].ravel(), child_rng[..., 1].ravel()
    ok_rng = ((0 <= f) & (f < e) & (e <= n)).reshape(nn, 2)
    fc, ec = np.clip(f, 0, n - 1), np.clip(e, 1, n)
    ec = np.maximum(ec, fc + 1)
    with np.errstate(all="ignore"):
        wlo = (_range_reduce(np.minimum, slo, fc, ec) - pad).reshape(nn, 2, 3)
        whi = (_range_reduce(np.maximum, shi, fc, ec) + pad).reshape(nn, 2, 3)
    if single:
        ok_rng[0, 1] = False
        if not (np.array_equal(_bits(blo[0, 1]), _bits([FLT_MAX] * 3)) and np.array_equal(_bits(bhi[0, 1]), _bits([-FLT_MAX] * 3))):
            out.add("binary.box", 0, 1, "the empty child is not behind an inverted box")
    bad = ((_bits(wlo) != _bits(blo)).any(2) | (_bits(whi) != _bits(bhi)).any(2)) & ok_rng
    out.add_where("binary.box", bad, np.arange(nn), "the child box is not the padded union of the triangles of its range")
    if nodes4 is None:
        return out

    # ---- the 4-wide nodes, in tandem with the collapse rule applied to `nodes`
    origin, stepw, qlo, qhi, refs4 = decode4(nodes4)
    n4 = len(origin)
    areas = child_areas(nodes if collapse_from is None else collapse_from).tolist()
    r4l = refs4.tolist()
    seen4 = [0] * n4
    at, src = [], []  # visited 4-wide nodes and their children by the rule
    stack = [(0, 0)]
    seen4[0] = 1
    while stack:
        i4, b = stack.pop()
        c = collapse_children(b, refs, areas)
        at.append(i4)
        src.append(c)
        for s in range(4):
            got = r4l[i4][s]
            if s >= len(c):
                if got != EMPTY_REF:
                    out.add("wide.unused", i4, s, "an unused slot with reference %d" % got)
                continue
            want_ref = refs[c[s][0]][c[s][1]]
            if want_ref < 0:
                if got != want_ref:
                    out.add("wide.child", i4, s, "reference %d where the collapse rule gives leaf %d" % (got, want_ref))
            elif not 0 <= got < n4:
                out.add("wide.child", i4, s, "reference %d where the collapse rule gives an inner node" % got)
            elif seen4[got]:
                seen4[got] += 1
                out.add("wide.reach", i4, s, "node %d reached %d times" % (got, seen4[got]))
            else:
                seen4[got] = 1
                stack.append((got, want_ref))
    for i4 in range(n4):
        if not seen4[i4]:
            out.add("wide.reach", i4, -1, "node %d not reached from the root" % i4)
    at = np.array(at, np.int64)
    m = len(at)
    used = np.zeros((m, 4), bool)
    sb, ss = np.zeros((m, 4), np.int64), np.zeros((m, 4), np.int64)
    for k, c in enumerate(src):
        for s, (nb, sd) in enumerate(c):
            used[k, s], sb[k, s], ss[k, s] = True, nb, sd
    origin, stepw, qlo, qhi = origin[at], stepw[at], qlo[at], qhi[at]
    unused_bad = ~used & ((qlo != 255).any(2) | (qhi != 0).any(2))
    out.add_where("wide.unused", unused_bad, at, "an unused slot without the inverted box (qlo 255, qhi 0)")
    expo = (stepw >> np.uint32(23)).astype(np.int64)
    step_bad = ((stepw & np.uint32(0x807FFFFF)) != 0) | (expo < 1) | (expo > 254)
    for k, a in zip(*np.nonzero(step_bad)):
        out.add("wide.step", at[k], -1, "axis %d: step word 0x%08x is no power of two with exponent in [1, 254]" % (a, stepw[k, a]))
    lo32, hi32 = blo[sb, ss], bhi[sb, ss]  # (m, 4, 3) the binary boxes of the children
    with np.errstate(all="ignore"):
        step = stepw.view(F).astype(np.float64)[:, None, :]
        o64 = origin.astype(np.float64)[:, None, :]
        plo, phi = o64 + qlo * step, o64 + qhi * step
        lo64, hi64 = lo32.astype(np.float64), hi32.astype(np.float64)
        u3 = used[:, :, None]
        out.add_where("wide.containment", u3 & (plo > lo64), at, "origin + qlo * step lies above the binary lo")
        out.add_where("wide.containment", u3 & (phi < hi64), at, "origin + qhi * step lies below the binary hi")
        omin = np.where(u3, lo32, F(np.inf)).min(1)
        H = np.where(u3, hi64, -np.inf).max(1)
        for k, a in zip(*np.nonzero(_bits(omin) != _bits(origin))):
            out.add("wide.tightness", at[k], -1, "axis %d: the origin is not the minimum of the children's lo" % a)
        out.add_where("wide.tightness", u3 & ~(lo64 - plo < step), at, "the lo plane lies a whole step or more below the binary lo")
        out.add_where("wide.tightness", u3 & ~(phi - hi64 < step), at, "the hi plane lies a whole step or more above the binary hi")
        bound = np.maximum(4.0 * (H - origin.astype(np.float64)) / 255.0, 2.0 ** -126)
        for k, a in zip(*np.nonzero(~(step[:, 0, :] <= bound))):
            out.add("wide.tightness", at[k], -1, "axis %d: step %g exceeds max(4 * extent / 255, 2^-126) = %g" % (a, step[k, 0, a], bound[k, a]))
        # ---- against the triangles directly: the decoded box of a child holds every vertex of every triangle of its slot range
        cr = child_rng[sb, ss]  # (m, 4, 2)
        ok = used & (cr[..., 0] >= 0) & (cr[..., 0] < cr[..., 1]) & (cr[..., 1] <= n)
        fc = np.clip(cr[..., 0], 0, n - 1).ravel()
        ec = np.maximum(np.clip(cr[..., 1], 1, n).ravel(), fc + 1)
        vlo = _range_reduce(np.minimum, slo.astype(np.float64), fc, ec).reshape(m, 4, 3)
        vhi = _range_reduce(np.maximum, shi.astype(np.float64), fc, ec).reshape(m, 4, 3)
        bad = ok[:, :, None] & ((plo > vlo) | (phi < vhi))
        out.add_where("wide.triangles", bad, at, "the decoded box does not hold every vertex of the triangles of its slot range")
    return out


# ------------------------------------------------------------------------------------------------ the cluster layout
def cluster_walk(w, c, root):
    """The cluster layout c (download_clusters, root entry `root`) walked level pair by level pair beside the 4-wide nodes w it was made from: every node
    appears once, with the same boxes; leaves keep their references; an even-level node is followed by its inner children in child order; the references of
    those to inner nodes are (slot << 4) | the mask of that node's inner children.  Asserts all of it; returns the number of levels walked."""
    REF = [10, 11, 12, 13]  # the four child references' columns (gvt_hip.h gvt_hip_mesh_download_wide)
    BOX = [i for i in range(16) if i not in REF]
    refs_w, refs_c = w[:, REF].view(np.int32), c[:, REF].view(np.int32)
    def inner_mask(r):  # (n, 4) int32 references -> bit c: child c is an inner node
        return ((r >= 0) * (1 << np.arange(4))).sum(1).astype(np.int64)
    seen = np.zeros(len(c), np.int64)
    wi, slot, mask = np.array([0], np.int64), np.array([root >> 4], np.int64), np.array([root & 15], np.int64)  # pairs (node of nodes4, its cluster's entry)
    levels = 0
    while len(wi):
        assert np.array_equal(w[wi][:, BOX], c[slot][:, BOX]) and np.array_equal(refs_w[wi] < 0, refs_c[slot] < 0)
        assert np.array_equal(mask, inner_mask(refs_w[wi]))
        leaf = refs_w[wi] < 0
        assert np.array_equal(refs_w[wi][leaf], refs_c[slot][leaf])
        np.add.at(seen, slot, 1)
        # the inner children: slot + 1 + (inner children before it)
        before = np.cumsum(~leaf, 1) - (~leaf)
        k, ch = np.nonzero(~leaf)
        cw, cs = refs_w[wi][k, ch].astype(np.int64), slot[k] + 1 + before[k, ch]
        assert np.array_equal(w[cw][:, BOX], c[cs][:, BOX])
        np.add.at(seen, cs, 1)
        rw, rc = refs_w[cw], refs_c[cs]
        gleaf = rw < 0
        assert np.array_equal(gleaf, rc < 0) and np.array_equal(rw[gleaf], rc[gleaf])
        k2, ch2 = np.nonzero(~gleaf)
        wi, ent = rw[k2, ch2].astype(np.int64), rc[k2, ch2].astype(np.int64)
        slot, mask = ent >> 4, ent & 15
        levels += 2
    assert np.all(seen == 1), "%d of %d cluster slots not reached exactly once" % (int((seen != 1).sum()), len(seen))
    return levels
