"""Meshes for the BVH structure tests (tests/bvh_checker.py): one seeded soup of mixed triangle sizes per size at which the builder changes route, and the
shapes that strain keys, ties, pads and quantisation at 1,025 triangles (table only) and 5,121 (chunks in LDS, a ragged last chunk).  No mesh holds a -0.0."""
import numpy as np

F = np.float32

# size -> what it exercises (lbvh.hip build_lbvh); 8,191 / 8,192 is where the key width really changes (key_bits: 18 + 3 per shift of n by 3)
SIZES = {
    1: "one node (k_single_node) under every leaf_max", 2: "one node from leaf_max 2", 3: "one node from leaf_max 4", 4: "one node at leaf_max 4",
    5: "the smallest tree under every leaf_max",
    31: "one table level", 32: "one table level, full", 33: "two table levels",
    1023: "two table levels", 1024: "two table levels, full", 1025: "three table levels",
    4095: "the last table-only build", 4096: "the first chunked build, full chunks", 4097: "a last chunk of one triangle",
    5121: "a ragged last chunk: 5 x 1,024 + 1",
    8191: "the last 30-bit keys", 8192: "the first 33-bit keys",
    33000: "four table levels, 33-bit keys",
}
SHAPES = ("coincident", "two-piles", "corner", "planar", "point", "box-1-2-4", "scale-1e30", "scale-1e-30", "scale-1e-34", "offset-1e6", "indexed")
SHAPE_SIZES = (1025, 5121)
CLUSTERED = ("coincident", "two-piles", "corner", "point")  # long runs of equal keys
TABLE_FORCED = (4097, 5121)
REFIT = (("soup", 5121), ("corner", 5121))


def _soup_points(n, rng):
    """(n, 3, 3) corners: centres uniform in the unit box, edge lengths from 3e-4 to 0.1 (log-uniform)."""
    c = rng.random((n, 1, 3))
    size = 10.0 ** rng.uniform(-3.5, -1.0, (n, 1, 1))
    return c + (rng.random((n, 3, 3)) - 0.5) * size


def _flat(p):
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    return p, np.arange(len(p), dtype=np.int32).reshape(-1, 3)


def soup(n, seed=None):
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    p = _soup_points(n, rng)
    if n >= 8192:
        # pairs of small triangles 1 / 1,500 apart: often in one cell of the 1,024^3 grid of 30-bit keys, in two cells of the 2,048^3 grid of 33-bit keys
        k = 512
        p[n - k:] = p[n - 2 * k:n - k] - np.array([1.0 / 1500.0, 0.0, 0.0])  # (the later triangle gets the lower key)
        p[n - 2 * k:] = p[n - 2 * k:].mean(1, keepdims=True) + (rng.random((2 * k, 3, 3)) - 0.5) * 1e-5
    return _flat(p)


def shape(name, n):
    rng = np.random.default_rng(abs(hash_name(name)) + n)
    if name == "coincident":  # split by position alone
        return np.array([[0.25, 0.5, 0.125], [0.75, 0.5, 0.25], [0.5, 0.875, 0.375]], F), np.tile(np.arange(3, dtype=np.int32), (n, 1))
    if name == "two-piles":  # two coincident piles far apart, alternating in the input
        v = np.array([[0.25, 0.5, 0.125], [0.375, 0.5, 0.25], [0.25, 0.625, 0.375], [900.0, 800.0, 700.0], [900.5, 800.0, 700.0], [900.0, 800.5, 700.25]], F)
        t = np.tile(np.arange(3, dtype=np.int32), (n, 1))
        t[1::2] += 3
        return v, t
    if name == "corner":  # 90 % of the triangles in a 1e-4 corner of the unit box
        k = (9 * n) // 10
        c = np.concatenate([rng.random((k, 1, 3)) * 1e-4, rng.random((n - k, 1, 3))])
        return _flat(c + (rng.random((n, 3, 3)) - 0.5) * 2e-5 + 1e-3)
    if name == "planar":  # one extent zero, boxes of zero thickness
        p = _soup_points(n, rng)
        p[..., 2] = 0.375
        return _flat(p)
    if name == "point":  # em = 0, iso = 0, every key 0
        return _flat(np.tile(np.array([0.3, 0.7, 0.2]), (n, 3, 1)))
    if name == "box-1-2-4":  # one scale for the three axes: the clamp stays inactive on the short ones
        return _flat(_soup_points(n, rng) * np.array([1.0, 2.0, 4.0]))
    if name == "scale-1e30":  # a large pad (areas overflow float32)
        return _flat(_soup_points(n, rng).astype(F) * F(1e30))
    if name == "scale-1e-30":  # a tiny pad, 1e-35: still a normal float
        return _flat(_soup_points(n, rng).astype(F) * F(1e-30))
    if name == "scale-1e-34":  # a pad that underflows: a subnormal (as are some edges; every area is 0)
        return _flat(_soup_points(n, rng).astype(F) * F(1e-34))
    if name == "offset-1e6":  # extent 1 at 1e6: the float spacing (1/16) is coarser than the quantisation steps
        return _flat(_soup_points(n, rng) + 1e6)
    if name == "indexed":  # shared vertices, unreferenced ones, one of them far outside the box
        g = int(np.ceil(np.sqrt(n / 2.0))) + 1
        x, y = np.meshgrid(np.arange(g), np.arange(g), indexing="ij")
        v = np.stack([x.ravel() / g, y.ravel() / g, 0.1 * np.sin(0.7 * x.ravel()) * np.cos(0.9 * y.ravel()) + 0.5], 1) + rng.random((g * g, 3)) * 1e-3
        i = (x[:-1, :-1] * g + y[:-1, :-1]).ravel()
        t = np.concatenate([np.stack([i, i + g, i + 1], 1), np.stack([i + 1, i + g, i + g + 1], 1)])[rng.permutation(2 * (g - 1) ** 2)[:n]]
        v = np.concatenate([[[50.0, -50.0, 50.0]], v, rng.random((7, 3)) * 0.5])  # unreferenced: vertex 0 and the last seven
        return np.ascontiguousarray(v, F), np.ascontiguousarray(t + 1, np.int32)
    raise KeyError(name)


def hash_name(name):
    return sum((k + 1) * ord(ch) for k, ch in enumerate(name))  # (hash() of a string changes from process to process)


def case(name, n):
    return soup(n) if name == "soup" else shape(name, n)
