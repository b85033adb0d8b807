"""The volume march (csrc/volume.hip) at its edges, bit for bit against the numpy checkers and against GVT_HIP_VOLUME_NO_SKIP: the cases
of tests/volume_edge_cases.py (tests/test_volume_edges_host.py shows on the CPU that they are not vacuous).  Plateaus next to single-entry
opacity spikes, NaN / Inf / huge samples, narrow ranges far from zero, values outside the table; sampling rates below 1 and anisotropic
spacing; origins on faces, edges, corners and vertices, zero / NaN / Inf rays, every kind of t_min, rays that arrive opaque; thin and
offset bricks traced directly and one after the other; samples handed over in device memory.  No tolerances anywhere."""
import numpy as np
import pytest

from gravit_amd import scenes
from gravit_amd.adapter import HipVolumeAdapter
from tests import volume_checker as vc
from tests import volume_edge_cases as ec
from tests import volume_surface_checker as sc
from tests.test_gpu_volume import IDENT, MOVED, grid, tf
from tests.test_gpu_volume_surfaces import LIGHTS, adapter, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
CASES = ec.skip_cases()
NONE = sc.Surfaces()


def checker(B, S, rays, minv):
    with np.errstate(all="ignore"):
        out = sc.march(B, S, rays, minv)
    return out, (sc.march.crossings if len(S) else 0)


def skip_and_not(vol, t, rate, S, rays, m=IDENT, must_skip=False):
    """One adapter that skips and one that does not: the same bits as each other and as the checker, for the rays and for their
    continuation; returns the skipping adapter's result."""
    minv = scenes.instance_matrices(m)[0]
    a, b = adapter(vol, t, rate, S, skip=True), adapter(vol, t, rate, S, skip=False)
    B = vc.Brick(vol, t, rate)
    ra, rb = a.trace(rays, m, minv), b.trace(rays, m, minv)
    want, crossings = checker(B, S, rays, minv)
    same_bits(ra, rb)
    same_bits(ra, want)
    ia, ib = a.info(), b.info()
    assert ia["samples_marched"] == ib["samples_marched"] == ib["samples_gathered"]
    assert a.crossings() == b.crossings() == crossings
    if must_skip:
        assert ia["n_blocks_empty"] > 0 and ia["samples_gathered"] < ia["samples_marched"]
    ra2, rb2 = a.trace(ra, m, minv), b.trace(rb, m, minv)  # the continuation: most rays own nothing more, the opaque ones one sample
    want2, crossings2 = checker(B, S, want, minv)
    same_bits(ra2, rb2)
    same_bits(ra2, want2)
    assert a.crossings() == b.crossings() == crossings + crossings2
    return ra


@pytest.fixture(scope="module")
def rays():
    return ec.edge_rays(ec.plateaus(), IDENT)


@pytest.mark.parametrize("name", sorted(CASES))
def test_skipping_gives_the_same_bits(hip, rays, name):
    vol, t, must_skip = CASES[name]
    got = skip_and_not(vol, t, 1.0, NONE, rays, must_skip=must_skip)
    assert ((got["depth"] & sc.SIDES) == 0).all()


PLATEAU_ISO = [(ec.PLATEAU_BLOCK + i) / 255.0 for i in (-1, 0, 1)]
INF_PLANE = [[1.0, 0.0, 0.0, -0.25], [0.3, 1.0, 0.1, 0.4]]  # x = the position of the vertices (4, ., .): through the block of the first Inf


@pytest.mark.parametrize("e", [78, 84, 177])
@pytest.mark.parametrize("half", [False, True])
def test_skipping_with_isovalues_on_the_plateaus(hip, rays, e, half):
    S = sc.Surfaces(PLATEAU_ISO, (), 0.4, LIGHTS[:1])
    got = skip_and_not(ec.plateaus(half), ec.spike(e), 1.0, S, rays, must_skip=True)
    assert ((got["depth"] & sc.SIDES) != 0).sum() > 500


@pytest.mark.parametrize("kind", ["pinf", "ninf", "nan", "mixed"])
@pytest.mark.parametrize("where", ["bottom", "top"])
@pytest.mark.parametrize("iso", [False, True])
def test_skipping_with_surfaces_on_nonfinite_samples(hip, rays, kind, where, iso):
    S = sc.Surfaces([0.25, 0.5] if iso else (), INF_PLANE, 0.4, LIGHTS[:2])
    skip_and_not(ec.nonfinite(kind), ec.nonfinite_table(where), 1.0, S, rays, must_skip=not iso)


def test_skipping_with_surfaces_on_huge_samples(hip, rays):
    S = sc.Surfaces([0.25, -1e38], INF_PLANE[:1], 0.4, LIGHTS[:1])
    skip_and_not(ec.huge(), ec.huge_table("low"), 1.0, S, rays)


# ---- rates and spacing
@pytest.mark.parametrize("rate", ec.RATES)
@pytest.mark.parametrize("which", ["plateaus-broad", "plateaus-84", "grid24"])
def test_sampling_rates(hip, which, rate):
    vol, t = {"plateaus-broad": (ec.plateaus(), ec.broad()), "plateaus-84": (ec.plateaus(), ec.spike(84)), "grid24": (grid(24), tf("cool"))}[which]
    r = ec.edge_rays(vol, IDENT, rate)
    skip_and_not(vol, t, rate, NONE, r, must_skip=which == "plateaus-84")
    # with surfaces: a brick that owns no sample of a ray leaves t_min, t and the SIDES flag as they came
    r["t"] = 123.0
    S = sc.Surfaces([0.3], [[0.0, 0.0, 1.0, 0.2]], 0.3, LIGHTS[:1])
    got = skip_and_not(vol, t, rate, S, r)
    unowned = (got["depth"] & sc.SIDES) == 0
    assert (got["t"][unowned] == 123.0).all() and (got["t_min"][unowned] == r["t_min"][unowned]).all() and (got["t"][~unowned] != 123.0).all()
    if rate == 0.11:
        tn, tf_ = vc.slab(*ec.box(vol), r["origin"], r["direction"])
        assert (unowned & (tn <= tf_) & (tf_ > r["t_min"]) & (tn > r["t_min"])).sum() >= 20  # ... although they cross its box


@pytest.mark.parametrize("rate", [0.37, 1.7])
@pytest.mark.parametrize("moved", [False, True])
def test_anisotropic_spacing(hip, rate, moved):
    vol = ec.volume(ec.plateaus().data, spacing=(1.0 / 16, 0.25 / 16, 3.0 / 16))
    m = MOVED if moved else IDENT
    r = ec.edge_rays(vol, m, rate)
    got = skip_and_not(vol, ec.broad(), rate, NONE, r, m)
    assert (got["w"] > 0).sum() > 300
    skip_and_not(vol, ec.spike(84), rate, sc.Surfaces(PLATEAU_ISO[:1], INF_PLANE[:1], 0.3, LIGHTS[:1]), r, m, must_skip=True)


# ---- ray edges
SURF = sc.Surfaces([0.42, 0.58], [[0.0, 0.0, 1.0, 0.4]], 0.15, LIGHTS[:1])


@pytest.mark.parametrize("which", ["plateaus", "grid24"])
@pytest.mark.parametrize("surf", [False, True])
def test_ray_edges_in_any_order_and_number(hip, which, surf):
    vol, t = (ec.plateaus(), ec.spike(84, 0.5)) if which == "plateaus" else (grid(24), tf("ramp"))
    S = SURF if surf else NONE
    for m in (IDENT, MOVED):
        minv = scenes.instance_matrices(m)[0]
        r = ec.edge_rays(vol, m, 1.7)
        r["t"] = 7.0
        ad = adapter(vol, t, 1.7, S)
        B = vc.Brick(vol, t, 1.7)
        want, _ = checker(B, S, r, minv)
        got = ad.trace(r, m, minv)
        same_bits(got, want)
        dead = ~np.isfinite(r["origin"]).all(axis=1) | ~np.isfinite(r["direction"]).all(axis=1) | (r["direction"] == 0).all(axis=1)
        assert dead.sum() >= 40 and (got["t_min"][dead] == r["t_min"][dead]).all() and (got["w"][dead] == 0).all()  # unmarched
        # another order: the same bits per id
        p = np.random.default_rng(5).permutation(len(r))
        again = ad.trace(r[p], m, minv)
        assert (again["id"] == r["id"][p]).all()
        same_bits(again, got[p])
        # a few sizes around a wave, and one lane
        for n in (1, 63, 64, 65, 257):
            same_bits(ad.trace(r[300:300 + n], m, minv), want[300:300 + n])


# ---- bricks through the trace entry point
@pytest.mark.parametrize("counts", [(2, 2, 2), (2, 9, 10), (17, 2, 2)])
def test_thin_volumes(hip, counts):
    vol = ec.thin(counts)
    r = ec.edge_rays(vol, IDENT, 1.7)
    got = skip_and_not(vol, tf("cool"), 1.7, NONE, r)
    assert (got["w"] > 0).sum() >= 100
    skip_and_not(vol, tf("spikes"), 1.7, SURF, r)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("rate", [0.37, 1.7])
@pytest.mark.parametrize("surf", [False, True])
def test_offset_bricks_one_after_the_other(hip, which, rate, surf):
    """Brick A, then the unfinished rays through its neighbour B (as the shuffle hands them on): each march equals the checker's on that
    brick, and the end equals one march through the union brick, the carried sides included."""
    a, b, u = ec.chain(ec.smooth(), which)
    t = ec.faint()
    S = SURF if surf else NONE
    r = ec.chain_rays(a, b, IDENT)
    r["t"] = 9.0
    first = skip_and_not(a, t, rate, S, r)
    go, on = ec.hop(first)
    second = first.copy()
    second[go] = skip_and_not(b, t, rate, S, on)
    whole = skip_and_not(u, t, rate, S, r)
    same_bits(second, whole)
    both = (first["t_min"] != r["t_min"]) & (second["t_min"] != first["t_min"])
    assert both.sum() >= 200 and (whole["w"] > 0).sum() >= 200
    # the edge rays straight at an offset brick (aimed at the global grid: many miss it, graze it or start inside it)
    skip_and_not(b, tf("spikes"), rate, S, ec.edge_rays(ec.smooth(), IDENT, rate))


# ---- samples in device memory
@pytest.mark.parametrize("name", ["plateaus-84", "nonfinite-mixed-bottom", "far_narrow"])
def test_device_samples(hip, rays, name):
    import torch

    vol, t, _ = CASES[name]
    b = ec.cut(vol, (1, 0, 2), (18, 10, 24))
    dev = scenes.Brick(torch.from_numpy(b.data).cuda(), b.offset, b.global_counts, b.origin, b.spacing, b.lo, b.hi)
    x, y = HipVolumeAdapter(dev, 1.0), HipVolumeAdapter(b, 1.0)
    for ad in (x, y):
        ad.set_transfer(t)
    rx, ry = x.trace(rays, IDENT, IDENT), y.trace(rays, IDENT, IDENT)
    same_bits(rx, ry)
    same_bits(rx, checker(vc.Brick(b, t, 1.0), NONE, rays, IDENT)[0])
    ix, iy = x.info(), y.info()
    for k in ix:
        assert np.array_equal(ix[k], iy[k], equal_nan=True), k
    assert ix["n_blocks_empty"] > 0 and ix["samples_gathered"] < ix["samples_marched"]
