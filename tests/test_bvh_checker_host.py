"""tests/bvh_checker.py checked without a device: the reference builder against a brute-force definition of Karras' tree, the validator on a valid tree
and on eleven damaged ones, and the conditions on tests/bvh_cases.py that the GPU tests (test_gpu_bvh_structure.py) rely on."""
import math

import numpy as np
import pytest

from tests import bvh_cases as cases
from tests import bvh_checker as chk

F = np.float32


# ------------------------------------------------------------------------------------------------ a valid 4-wide layout, built on the host
def quantise_host(lo, hi):
    """Outward-rounding quantiser in float64, for this test only: lo, hi (k, 3) float32 child boxes -> origin (3,) float32, exponents (3,), qlo, qhi
    (k, 3).  The smallest power-of-two step whose 255 steps reach every hi plane; lo planes rounded down, hi planes rounded up."""
    o = lo.min(0)
    lo64, hi64, o64 = lo.astype(np.float64), hi.astype(np.float64), o.astype(np.float64)
    ex, qlo, qhi = np.zeros(3, np.int64), np.zeros(lo.shape, np.int64), np.zeros(lo.shape, np.int64)
    for a in range(3):
        ext = float(hi64[:, a].max() - o64[a])
        e = 1 if ext <= 0 else min(max(math.frexp(ext / 255.0)[1] - 1 + 127, 1), 254)
        while True:
            step = 2.0 ** (e - 127)
            l, u = np.floor((lo64[:, a] - o64[a]) / step), np.ceil((hi64[:, a] - o64[a]) / step)
            if u.max() <= 255 or e >= 254:
                break
            e += 1
        assert (o64[a] + l * step <= lo64[:, a]).all() and (o64[a] + u * step >= hi64[:, a]).all()  # (exact: a few bits of quotient, a power-of-two step)
        ex[a], qlo[:, a], qhi[:, a] = e, l, u
    return o, ex, qlo, qhi


def wide_host(nodes, collapse_from=None):
    """nodes4 (m, 16) uint32 of a binary tree: the collapse rule breadth first (by the areas of collapse_from's boxes, when given: the 4-wide topology a
    refit keeps), every node quantised by quantise_host."""
    nodes = np.ascontiguousarray(nodes, F)
    refs = nodes.view(np.int32)[:, 12:14].tolist()
    areas = chk.child_areas(nodes if collapse_from is None else collapse_from).tolist()
    lo, hi = chk._child_planes(nodes)
    rows, queue = [], [0]
    while len(rows) < len(queue):
        c = chk.collapse_children(queue[len(rows)], refs, areas)
        w = np.zeros(16, np.uint32)
        r = np.full(4, -1, np.int32)
        for s, (nb, sd) in enumerate(c):
            r[s] = refs[nb][sd]
            if r[s] >= 0:
                queue.append(int(r[s]))
                r[s] = len(queue) - 1
        o, ex, qlo, qhi = quantise_host(np.stack([lo[nb, sd] for nb, sd in c]), np.stack([hi[nb, sd] for nb, sd in c]))
        w[0:3] = o.view(np.uint32)
        w[[3, 14, 15]] = (ex << 23).astype(np.uint32)
        for a in range(3):
            ql = sum(int(qlo[s, a]) << (8 * s) for s in range(len(c))) | sum(255 << (8 * s) for s in range(len(c), 4))
            w[4 + 2 * a], w[5 + 2 * a] = ql, sum(int(qhi[s, a]) << (8 * s) for s in range(len(c)))
        w[10:14] = r.view(np.uint32)
        rows.append(w)
    return np.stack(rows)


# ------------------------------------------------------------------------------------------------ the reference against a brute-force definition
SMALL = [("soup", 2), ("soup", 5), ("soup", 33), ("soup", 200), ("corner", 200), ("coincident", 150), ("two-piles", 101), ("point", 64), ("planar", 120),
         ("indexed", 97)]


@pytest.mark.parametrize("name,n", SMALL)
def test_reference_topology_is_karras_tree_by_brute_force(name, n):
    """Every inner node i of the reference: its range is the maximal run of positions around i that share more with position i than i's nearer-prefix
    neighbour does, its split lies behind the one adjacent pair that differs in the range's first differing bit -- all recomputed by loops over all pairs;
    and the order is "sorted by (key, primID)"."""
    v, t = cases.case(name, n)
    T = chk.karras_topology(v, t, 1)
    tlo, thi = chk.tri_boxes(v, t)
    lo, _, iso, _ = chk.scene_record(tlo, thi)
    keys = chk.morton_keys(tlo, thi, lo, iso, T.key_bits)
    assert T.key_bits == 30 and all(0 <= k < 1 << 30 for k in keys)
    pairs = sorted((keys[p], p) for p in range(n))
    assert [p for _, p in pairs] == T.order.tolist() and [k for k, _ in pairs] == T.keys
    K = T.keys

    def d(i, j):  # the kernel's delta, out-of-range positions included
        if j < 0 or j >= n:
            return -1
        if K[i] == K[j]:
            return 64 + 32 - (i ^ j).bit_length() if i != j else 10 ** 9
        return 64 - (K[i] ^ K[j]).bit_length()

    assert len(T.first) == n - 1
    for i in range(n - 1):
        dmin = min(d(i, i - 1), d(i, i + 1))
        run = [k for k in range(n) if d(i, k) > dmin]
        assert run == list(range(run[0], run[-1] + 1)) and i in (run[0], run[-1]) and len(run) >= 2
        prefix = min(d(a, b) for a in run for b in run if a != b)
        split = [g for g in run[:-1] if d(g, g + 1) == prefix]
        assert len(split) == 1
        assert (T.first[i], T.last[i], T.gamma[i]) == (run[0], run[-1], split[0]), i
    # the node numbering: a range's node is its first or its last position; the children are gamma and gamma + 1
    assert T.first[0] == 0 and T.last[0] == n - 1
    for i in range(n - 1):
        g = int(T.gamma[i])
        if g > T.first[i]:
            assert (T.first[g], T.last[g]) == (T.first[i], g)
        if g + 1 < T.last[i]:
            assert (T.first[g + 1], T.last[g + 1]) == (g + 1, T.last[i])


@pytest.mark.parametrize("leaf_max", [1, 2, 4])
@pytest.mark.parametrize("name,n", [("soup", 1), ("soup", 4), ("soup", 5), ("soup", 33), ("soup", 1025), ("corner", 1025), ("coincident", 1025), ("point", 1025),
                                    ("planar", 1025), ("scale-1e30", 1025), ("scale-1e-30", 1025), ("scale-1e-34", 1025), ("offset-1e6", 1025), ("indexed", 1025), ("soup", 4097)])
def test_validator_accepts_the_reference_tree(name, n, leaf_max):
    v, t = cases.case(name, n)
    R = chk.reference_tree(v, t, leaf_max)
    assert R.n_nodes == len(R.nodes) and R.nodes.shape[1] == 16 and R.slots.shape == (n, 16)
    assert chk.validate(v, t, R.nodes, wide_host(R.nodes), R.slots, leaf_max) == []
    if n > leaf_max:  # compaction: a live node's index is the number of live nodes before it
        live = (R.topology.last - R.topology.first + 1) > leaf_max
        assert R.n_nodes == int(live.sum()) and R.n_leaves == R.n_nodes + 1


def test_validator_accepts_a_refitted_tree_under_the_builds_collapse():
    """A refit keeps the topology, binary and 4-wide, of the build: the old vertices' tree with the new vertices' boxes is valid when the walk follows the
    collapse that the BUILD's areas chose -- and that collapse is not the one the new boxes would choose."""
    v, t = cases.soup(1025)
    rng = np.random.default_rng(5)
    nv = (v + rng.normal(scale=0.01, size=v.shape)).astype(F)
    old = chk.reference_tree(v, t, 2)
    new = chk.reference_tree(nv, t, 2, topology=old.topology)
    assert np.array_equal(old.nodes.view(np.int32)[:, 12:14], new.nodes.view(np.int32)[:, 12:14]) and not np.array_equal(old.nodes, new.nodes)
    assert np.array_equal(old.slots.view(np.int32)[:, 3], new.slots.view(np.int32)[:, 3])
    W = wide_host(new.nodes, collapse_from=old.nodes)
    assert chk.validate(nv, t, new.nodes, W, new.slots, 2, collapse_from=old.nodes) == []
    assert "wide.child" in {f.rule for f in chk.validate(nv, t, new.nodes, W, new.slots, 2)}


# ------------------------------------------------------------------------------------------------ the validator on damaged trees
@pytest.fixture(scope="module")
def tree1025():
    v, t = cases.soup(1025)
    R = chk.reference_tree(v, t, 2)
    W = wide_host(R.nodes)
    assert chk.validate(v, t, R.nodes, W, R.slots, 2) == []
    return v, t, R.nodes, W, R.slots


def _leaf_child(nodes, count):
    refs = nodes.view(np.int32)[:, 12:14]
    k, s = np.nonzero((refs < 0) & ((~refs & 7) == count))
    return int(k[len(k) // 2]), int(s[len(k) // 2])


def m_binary_hi_ulp(nodes, wide, slots):
    nodes[5, 1] = np.nextafter(nodes[5, 1], F(-np.inf))


def m_qhi_lowered(nodes, wide, slots):
    assert (wide[0, 5] >> 8) & 255 > 0
    wide[0, 5] -= 1 << 8  # child 1, x


def m_qlo_raised(nodes, wide, slots):
    assert (wide[0, 6] >> 16) & 255 < 255
    wide[0, 6] += 1 << 16  # child 2, y


def m_step_exponent(nodes, wide, slots):
    wide[3, 14] += 2 << 23


def m_origin_lowered(nodes, wide, slots):
    o, step = wide[2:3, 0].view(F), wide[2:3, 3].view(F)
    o[0] = o[0] - F(100) * step[0]


def m_slots_swapped(nodes, wide, slots):
    slots[[0, len(slots) - 1]] = slots[[len(slots) - 1, 0]]


def m_leaf_count_raised(nodes, wide, slots):
    k, s = _leaf_child(nodes, 1)
    nodes.view(np.int32)[k, 12 + s] = ~(~nodes.view(np.int32)[k, 12 + s] + 1)


def m_reference_emptied(nodes, wide, slots):
    wide[1, 10] = 0xFFFFFFFF


def m_shared_child(nodes, wide, slots):
    refs = nodes.view(np.int32)[:, 12:14]
    k = np.nonzero(refs[:, 0] >= 0)[0]
    refs[k[3], 0] = refs[k[7], 0]


def m_leaf_too_large(nodes, wide, slots):
    k, s = _leaf_child(nodes, 2)
    nodes.view(np.int32)[k, 12 + s] = ~(~nodes.view(np.int32)[k, 12 + s] + 1)  # 3 triangles under leaf_max 2


def m_primid_duplicated(nodes, wide, slots):
    slots.view(np.int32)[40, 3] = slots.view(np.int32)[41, 3]


MUTATIONS = [
    (m_binary_hi_ulp, "binary.box"), (m_qhi_lowered, "wide.containment"), (m_qlo_raised, "wide.containment"), (m_step_exponent, "wide.tightness"),
    (m_origin_lowered, "wide.tightness"), (m_slots_swapped, "wide.triangles"), (m_leaf_count_raised, "binary.tiling"), (m_reference_emptied, "wide.child"),
    (m_shared_child, "binary.reach"), (m_leaf_too_large, "binary.leaf_size"), (m_primid_duplicated, "slots.permutation"),
]


@pytest.mark.parametrize("mutate,rule", MUTATIONS, ids=[m.__name__[2:] for m, _ in MUTATIONS])
def test_validator_rejects_a_damaged_tree(tree1025, mutate, rule):
    """One element of a valid 1,025-triangle tree damaged: the validator reports it under the rule that the damage breaks, at a node and a slot."""
    v, t, nodes, wide, slots = tree1025
    nodes, wide, slots = nodes.copy(), wide.copy(), slots.copy()
    mutate(nodes, wide, slots)
    found = chk.validate(v, t, nodes, wide, slots, 2)
    hit = [f for f in found if f.rule == rule]
    assert hit, "expected a finding of %s, got %s" % (rule, found)
    assert all(isinstance(f.node, int) and isinstance(f.slot, int) and f.detail for f in found)


def test_mutations_name_the_damaged_element(tree1025):
    v, t, nodes, wide, slots = tree1025
    n2, w2 = nodes.copy(), wide.copy()
    m_binary_hi_ulp(n2, w2, None)
    m_qhi_lowered(n2, w2, None)
    found = chk.validate(v, t, n2, w2, slots, 2)
    assert ("binary.box", 5, 0) in [(f.rule, f.node, f.slot) for f in found]
    assert ("wide.containment", 0, 1) in [(f.rule, f.node, f.slot) for f in found]


# ------------------------------------------------------------------------------------------------ what the GPU tests rely on
def test_sizes_take_every_route():
    sizes = set(cases.SIZES)
    assert {1, 2, 3, 4, 5, 31, 32, 33, 1023, 1024, 1025, 4095, 4096, 4097, 5121, 33000} <= sizes
    for leaf_max in (1, 2, 4):  # one node, and the smallest tree behind it
        assert leaf_max in sizes and leaf_max + 1 in sizes
    assert [chk.table_levels(n) for n in (31, 32, 33, 1023, 1024, 1025, 4095, 33000)] == [1, 1, 2, 2, 2, 3, 3, 4]
    assert max(n for n in sizes if n < chk.CHUNKED_FROM) == chk.CHUNKED_FROM - 1 and chk.CHUNKED_FROM in sizes
    assert 4097 % chk.NB_CHUNK == 1 and 5121 % chk.NB_CHUNK == 1 and 4096 % chk.NB_CHUNK == 0
    assert set(cases.TABLE_FORCED) <= sizes and all(n >= chk.CHUNKED_FROM for n in cases.TABLE_FORCED)
    assert min(cases.SHAPE_SIZES) < chk.CHUNKED_FROM <= max(cases.SHAPE_SIZES)
    # the key width: 30 bits up to 8,191 triangles, 33 from 8,192 (not from 32,768: key_bits counts the shifts of n by 3 until it REACHES 1)
    assert [chk.key_bits(n) for n in (1, 5, 4097, 8191, 8192, 32767, 32768, 33000, 65535, 65536)] == [30, 30, 30, 30, 33, 33, 33, 33, 33, 36]
    assert {8191, 8192} <= sizes


@pytest.mark.parametrize("n", cases.SHAPE_SIZES)
@pytest.mark.parametrize("name", cases.CLUSTERED)
def test_clustered_cases_hold_long_runs_of_equal_keys(name, n):
    v, t = cases.shape(name, n)
    K = chk.karras_topology(v, t, 1).keys
    best = run = 1
    ends = []
    for i in range(1, n):
        run = run + 1 if K[i] == K[i - 1] else 1
        if run >= 64 and (i + 1 == n or K[i + 1] != K[i]):
            ends.append((i + 1 - run, i))
        best = max(best, run)
    assert best >= 64
    if n >= chk.CHUNKED_FROM:  # ... inside and across chunk boundaries
        assert any(a // chk.NB_CHUNK != b // chk.NB_CHUNK for a, b in ends)
    if name == "point":
        assert set(K) == {0}


def test_cases_are_what_they_claim():
    for n in cases.SHAPE_SIZES:
        for name in cases.SHAPES:
            v, t = cases.shape(name, n)
            assert len(t) == n and v.dtype == F and t.dtype == np.int32 and t.min() >= 0 and t.max() < len(v)
            assert not np.signbit(v[v == 0]).any() and np.isfinite(v).all()
        tlo, thi = chk.tri_boxes(*cases.shape("point", n))
        lo, hi, iso, pad = chk.scene_record(tlo, thi)
        assert iso == 0 and pad > 0 and (lo == hi).all()
        tlo, thi = chk.tri_boxes(*cases.shape("planar", n))
        assert (tlo[:, 2] == thi[:, 2]).all()
        tlo, thi = chk.tri_boxes(*cases.shape("scale-1e-30", n))
        assert np.finfo(F).tiny < chk.scene_record(tlo, thi)[3] < 2e-35
        tlo, thi = chk.tri_boxes(*cases.shape("scale-1e-34", n))
        assert 0 < chk.scene_record(tlo, thi)[3] < np.finfo(F).tiny  # the pad is a subnormal
        v, t = cases.shape("indexed", n)
        used = np.zeros(len(v), bool)
        used[t.ravel()] = True
        assert (~used).sum() >= 2 and not used[0] and np.bincount(t.ravel()).max() >= 3
        lo, hi, _, _ = chk.scene_record(*chk.tri_boxes(v, t))
        assert (v[0] > hi).any() or (v[0] < lo).any()  # the far vertex would move the scene box if it counted
        v, t = cases.shape("offset-1e6", n)
        assert np.all(v >= 1e6) and np.all(np.spacing(v) == F(0.0625))
    for n in cases.SIZES:
        assert len(cases.soup(n)[1]) == n


@pytest.fixture(scope="module")
def soup33000():
    return cases.soup(33000)


def test_the_largest_soup_needs_its_33_bit_keys(soup33000):
    v, t = soup33000
    assert chk.key_bits(len(t)) == 33
    tlo, thi = chk.tri_boxes(v, t)
    lo, _, iso, _ = chk.scene_record(tlo, thi)
    k33 = np.array(chk.morton_keys(tlo, thi, lo, iso, 33), np.uint64)
    k30 = np.array(chk.morton_keys(tlo, thi, lo, iso, 30), np.uint64)
    assert np.array_equal(k30, k33 >> np.uint64(3))
    o = np.argsort(k33, kind="stable")
    a, b = o[:-1], o[1:]
    tied_at_30 = (k30[a] == k30[b]) & (k33[a] != k33[b])
    assert tied_at_30.sum() >= 1
    # ... and at least one such pair stands in the other order than a 30-bit sort (ties by primID) would leave it
    assert (a[tied_at_30] > b[tied_at_30]).any()
