"""The BVH builder (gravit_amd/csrc/lbvh.hip) against an independent reference tree and against the triangles themselves.

For every size at which the builder changes route, for the shapes that strain keys, ties, pads and quantisation, and for leaf_max 1, 2 and 4: the binary
nodes and the triangle slots of a build equal tests/bvh_checker.py's reference IN EVERY BIT (boxes, references, order), the mesh's info equals the
reference's, and the validator has no finding on the device's 4-wide nodes -- containment and tightness of every quantised plane in float64, and every
decoded box against the vertices of the triangles below it.  The same for the route that takes every node box from the range-union table, and for refits
(the old vertices' topology, the new vertices' boxes).  No tolerance anywhere: equalities are exact, inequalities are the bounds that follow from quantise4.

Routes covered: the single node (n <= leaf_max); range-union tables of one to four levels (n = 31 / 32 / 33, 1,023 / 1,024 / 1,025, 33,000); the last
table-only build (4,095) and the chunked builds in LDS with their spine lists (4,096 full chunks, 4,097 and 5,121 with a last chunk of one triangle);
30-bit keys and 33-bit keys.  The key width changes at 8,192 triangles, not at 32,768 -- build_lbvh adds 3 bits per shift of n by 3 until n REACHES 1 --
so 8,191 and 8,192 stand beside the 33,000 of the plan.

Deliberately not covered: a fifth and sixth table level (n > 32^4); trees beyond 2^26 nodes; coordinates whose extent overflows float32.  Neither are
zeros of mixed sign or NaN coordinates (the order of min / max over them is not modelled)."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library initialises the device, as in test_gpu_animation.py)

from gravit_amd import scenes
from gravit_amd.adapter import HipMeshAdapter
from tests import bvh_cases as cases
from tests import bvh_checker as chk
from tests.test_gpu_animation import deform

pytestmark = pytest.mark.gpu

F = np.float32
LEAF_MAX = (1, 2, 4)
LEAF_MAX_DEFAULT = 2


class Trees:
    """Meshes and reference topologies, computed once per session (the 33,000-triangle one takes the longest) and never changed."""

    def __init__(self):
        self.meshes, self.topologies = {}, {}

    def mesh(self, name, n):
        if (name, n) not in self.meshes:
            v, t = cases.case(name, n)
            v.setflags(write=False)
            t.setflags(write=False)
            self.meshes[name, n] = (v, t)
        return self.meshes[name, n]

    def topology(self, name, n, leaf_max):
        key = (name, n, leaf_max if n <= chk.LEAF_MAX_LIMIT else 0)  # (the tree itself depends on leaf_max only through the single-node case)
        if key not in self.topologies:
            self.topologies[key] = chk.karras_topology(*self.mesh(name, n), leaf_max)
        T = self.topologies[key]
        T.leaf_max = leaf_max
        T.single = n <= leaf_max
        return T

    def reference(self, name, n, leaf_max, verts=None):
        v, t = self.mesh(name, n)
        return chk.reference_tree(v if verts is None else verts, t, leaf_max, topology=self.topology(name, n, leaf_max))


@pytest.fixture(scope="module")
def trees():
    return Trees()


def build(hip, v, t, leaf_max):
    try:
        hip.set_option("leaf_max", leaf_max)
        return HipMeshAdapter(scenes.MeshData(np.ascontiguousarray(v, F), np.ascontiguousarray(t, np.int32)))
    finally:
        hip.set_option("leaf_max", LEAF_MAX_DEFAULT)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def first_difference(a, b):
    if a.shape != b.shape:
        return "shapes %s and %s" % (a.shape, b.shape)
    k = np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(1))[0]
    return "" if not len(k) else "%d rows differ, the first is row %d:\n device    %s\n reference %s\n (as floats: %s | %s)" % (
        len(k), k[0], a.view(np.uint32)[k[0]], b.view(np.uint32)[k[0]], a[k[0]], b[k[0]])


def assert_tree(ad, R, v, t, leaf_max, collapse_from=None):
    nodes = ad.download_nodes()
    wide, slots = ad.download_wide()
    assert same_bits(slots, R.slots), "slots: " + first_difference(slots, R.slots)
    assert same_bits(nodes, R.nodes), "binary nodes: " + first_difference(nodes, R.nodes)
    found = chk.validate(v, t, nodes, wide, slots, leaf_max, collapse_from=collapse_from)
    assert found == [], "\n".join(map(str, found))
    i = ad.info()
    assert same_bits(np.array(i["bbox_lo"], F), R.bbox_lo) and same_bits(np.array(i["bbox_hi"], F), R.bbox_hi)
    assert (i["n_tris"], i["n_nodes"], i["max_leaf"]) == (len(t), R.n_nodes, leaf_max)
    assert i["n_leaves"] == R.n_leaves
    assert same_bits(np.array([i["sah_inner"]], F), np.array([R.sah_inner], F)), (i["sah_inner"], R.sah_inner)
    assert i["packet"] == R.packet
    return wide


@pytest.mark.parametrize("leaf_max", LEAF_MAX)
@pytest.mark.parametrize("n", sorted(cases.SIZES))
def test_soup_build_equals_the_reference_tree(hip, trees, n, leaf_max):
    """A seeded soup of mixed triangle sizes at every size where the builder changes route (tests/bvh_cases.py SIZES says which)."""
    v, t = trees.mesh("soup", n)
    R = trees.reference("soup", n, leaf_max)
    assert (R.n_nodes == 1 and R.nodes.view(np.int32)[0, 13] == -1) == (n <= leaf_max)
    ad = build(hip, v, t, leaf_max)
    try:
        assert_tree(ad, R, v, t, leaf_max)
    finally:
        ad.close()


@pytest.mark.parametrize("leaf_max", LEAF_MAX)
@pytest.mark.parametrize("n", cases.SHAPE_SIZES)
@pytest.mark.parametrize("name", cases.SHAPES)
def test_shape_build_equals_the_reference_tree(hip, trees, name, n, leaf_max):
    """Coincident triangles (split by position alone), two piles, a crowded corner (runs of equal keys inside and across chunks), a plane (boxes of zero
    thickness), a point (iso = 0, every key 0), a 1 : 2 : 4 box, coordinates around 1e30, 1e-30 and 1e-34 (a subnormal pad), extent 1 at 1e6 (float
    spacing coarser than the quantisation step), and an indexed mesh with shared and unreferenced vertices -- without (1,025) and with (5,121) chunks."""
    v, t = trees.mesh(name, n)
    R = trees.reference(name, n, leaf_max)
    ad = build(hip, v, t, leaf_max)
    try:
        assert_tree(ad, R, v, t, leaf_max)
    finally:
        ad.close()


@pytest.mark.parametrize("leaf_max", LEAF_MAX)
@pytest.mark.parametrize("name,n", [("soup", n) for n in cases.TABLE_FORCED] + [("corner", 5121)])
def test_table_forced_build_equals_the_reference_tree(hip, trees, name, n, leaf_max, monkeypatch):
    """Every node box from the range-union table (GVT_HIP_NODE_BOXES_TABLE) at sizes that otherwise go through the chunks: the same array as the
    reference, not merely the same as the other route."""
    v, t = trees.mesh(name, n)
    R = trees.reference(name, n, leaf_max)
    monkeypatch.setenv("GVT_HIP_NODE_BOXES_TABLE", "1")
    ad = build(hip, v, t, leaf_max)
    try:
        assert_tree(ad, R, v, t, leaf_max)
    finally:
        ad.close()


@pytest.mark.parametrize("leaf_max", LEAF_MAX)
@pytest.mark.parametrize("kind", ["jitter", "permute"])
@pytest.mark.parametrize("name,n", cases.REFIT)
def test_refit_keeps_the_topology_and_takes_the_new_boxes(hip, trees, name, n, kind, leaf_max):
    """update_vertices: the topology of the OLD vertices, the boxes, the pad and the slots of the NEW ones -- every bit of the binary nodes and the
    slots; no finding on the refitted 4-wide nodes (the build's collapse, the new boxes); and the cluster layout, laid out again, is still the same tree."""
    v, t = trees.mesh(name, n)
    nv = deform(v, kind)
    assert nv.shape == v.shape and not np.array_equal(nv, v)
    R = trees.reference(name, n, leaf_max, verts=nv)
    built = trees.reference(name, n, leaf_max).nodes  # (the 4-wide children were chosen by the areas of the build's boxes)
    ad = build(hip, v, t, leaf_max)
    try:
        c, root = ad.download_clusters()  # (built on first use: the refit lays it out again)
        assert c is not None
        ad.update_vertices(nv)
        wide = assert_tree(ad, R, nv, t, leaf_max, collapse_from=built)
        c, root = ad.download_clusters()
        assert c is not None and c.shape == wide.shape and root >> 4 == 0
        assert chk.cluster_walk(wide, c, root) <= 32
    finally:
        ad.close()


@pytest.mark.parametrize("name,n", [("point", 1025), ("scale-1e-30", 1025), ("scale-1e-30", 5121), ("soup", 5), ("soup", 2)])
def test_refit_of_unchanged_vertices_keeps_the_info_of_the_build(hip, trees, name, n):
    """Where the scene box has no area -- a point, or extents whose products underflow -- the packet statistic has no denominator: the build reports
    sah_inner = 1 (an empty sum) and so does a refit, which must give the build's tree and the build's info back for unchanged vertices (refit_lbvh used
    to leave sah_inner = 0 and the packets off there).  The single node (soup of 2) and the smallest tree (soup of 5) go through the same round trip."""
    v, t = trees.mesh(name, n)
    R = trees.reference(name, n, LEAF_MAX_DEFAULT)
    if n > 5:
        ex = R.bbox_hi - R.bbox_lo
        assert ex[0] * ex[1] + ex[1] * ex[2] + ex[2] * ex[0] == 0 and R.sah_inner == 1 and R.packet == 1
    ad = build(hip, v, t, LEAF_MAX_DEFAULT)
    try:
        assert_tree(ad, R, v, t, LEAF_MAX_DEFAULT)
        ad.update_vertices(v)
        assert_tree(ad, R, v, t, LEAF_MAX_DEFAULT)
    finally:
        ad.close()
