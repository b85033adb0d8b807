"""The inputs of tests/test_gpu_volume_edges.py are not vacuous: with the numpy checker alone (no GPU), the "must skip" pairs have
macro cells that are empty and rays that sample them, the non-finite volumes produce NaN samples that the table shows, every
sampling rate leaves both translucent and finished rays, and the checker agrees with itself across thin and offset bricks."""
import numpy as np
import pytest

from tests import volume_checker as vc
from tests import volume_edge_cases as ec
from tests import volume_surface_checker as sc
from tests.test_gpu_volume import IDENT, grid, tf

F = np.float32
CASES = ec.skip_cases()
MUST_SKIP = sorted(k for k, v in CASES.items() if v[2])


def bits(a, b, fields):
    for f in fields:
        x, y = np.ascontiguousarray(a[f]).view(np.uint32), np.ascontiguousarray(b[f]).view(np.uint32)
        assert (x == y).all(), f


@pytest.fixture(scope="module")
def rays():
    return ec.edge_rays(ec.plateaus(), IDENT)


def test_the_ray_list(rays):
    assert 1900 <= len(rays) <= 2100 and sorted(rays["id"]) == list(range(len(rays)))
    d, o = rays["direction"], rays["origin"]
    lo, hi = ec.box(ec.plateaus())
    assert ((d == 0).all(axis=1)).sum() >= 8 and np.isnan(d).any() and np.isnan(o).any() and np.isinf(d).any() and np.isinf(o).any()
    for edge in (lo, hi):  # the inclusive slab test: a zero direction component with the origin exactly on the face
        assert (((o == edge) & (d == 0)).any(axis=1)).sum() >= 20
    assert ((o == lo).all(axis=1)).sum() >= 5 and ((o == hi).all(axis=1)).sum() >= 5
    assert (rays["t_min"] < 0).sum() >= 40 and (rays["t_min"] == F(1e30)).sum() == 20
    for w in (0.98999, 0.99, 1.0):
        assert (rays["w"] == F(w)).sum() == 60
    # rays through grid vertices: all three fractions are exactly 0 at some owned sample
    B = vc.Brick(ec.plateaus(), ec.broad(), 1.0)
    j, k, c, v = ec.owned_samples(B, rays, IDENT)
    own, _, f = vc.cells(B, rays["origin"][j], rays["direction"][j], k)
    assert own.all() and len(np.unique(j[(f == 0).all(axis=1)])) >= 100
    # and the permutation interleaves them: no wave of 64 is all dead or all alive
    alive = np.isin(np.arange(len(rays)), j)
    per_wave = [alive[s:s + 64].sum() for s in range(0, len(rays) - 63, 64)]
    assert min(per_wave) >= 8 and max(per_wave) <= 60


@pytest.mark.parametrize("name", MUST_SKIP)
def test_must_skip_pairs_have_empty_blocks_and_rays_in_them(rays, name):
    vol, t, _ = CASES[name]
    B = vc.Brick(vol, t, 1.0)
    through, cand = ec.rays_through_empty_blocks(B, rays, IDENT)
    assert cand.sum() >= 1
    assert len(through) >= 200


@pytest.mark.parametrize("kind", ["pinf", "ninf", "nan", "mixed"])
def test_nonfinite_volumes_give_nan_samples_the_table_shows(rays, kind):
    B = vc.Brick(ec.nonfinite(kind), ec.nonfinite_table("bottom"), 1.0)
    j, k, c, v = ec.owned_samples(B, rays, IDENT)
    nan = np.isnan(v)
    assert nan.sum() >= 50
    assert (ec.opacity_at(B, v[nan]) > 0).sum() >= 10


def test_huge_neighbours_overflow_the_lerp(rays):
    B = vc.Brick(ec.huge(), ec.huge_table("low"), 1.0)
    j, k, c, v = ec.owned_samples(B, rays, IDENT)
    bad = ~np.isfinite(v)
    assert np.isfinite(B.vox).all() and bad.sum() >= 50
    assert (ec.opacity_at(B, v[bad]) > 0).sum() >= 10


def test_far_narrow_blocks_lie_between_the_spikes():
    B = vc.Brick(ec.far_narrow(), ec.far_narrow_table(), 1.0)
    cand = ec.candidate_empty_blocks(B)
    assert cand[0].all() and cand[2].all() and cand[3].all() and not cand[1].any()


@pytest.mark.parametrize("rate", ec.RATES)
@pytest.mark.parametrize("which", ["plateaus", "grid24"])
def test_every_rate_leaves_translucent_and_finished_rays(which, rate):
    vol, t = (ec.plateaus(), ec.broad()) if which == "plateaus" else (grid(24), tf("cool"))
    r = ec.edge_rays(vol, IDENT, rate)
    with np.errstate(all="ignore"):
        got = vc.march(vc.Brick(vol, t, rate), r, IDENT)
    fresh = r["w"] == 0
    assert (got["w"][fresh] > 0).sum() >= 100
    assert ((got["depth"] & vc.BOUNDARY) != 0).sum() >= 100
    if rate == 0.11:  # a step is longer than a macro cell: some rays cross the box and own no sample in it
        tn, tf_ = vc.slab(*ec.box(vol), r["origin"], r["direction"])
        crossed = (tn <= tf_) & (tf_ > r["t_min"]) & (tn > r["t_min"])
        assert (crossed & (got["t_min"] == r["t_min"])).sum() >= 20


SURF = sc.Surfaces([0.42, 0.58], [[0.0, 0.0, 1.0, 0.4]], 0.15, [((3.0, 4.0, 5.0), (1.0, 0.9, 0.8))])


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("rate", [0.37, 1.7])
@pytest.mark.parametrize("surf", [False, True])
def test_the_checker_agrees_with_itself_across_offset_bricks(which, rate, surf):
    """March brick A, then the rays that are not finished through its neighbour B: the bits of one march through the union brick."""
    a, b, u = ec.chain(ec.smooth(), which)
    t = ec.faint()
    r = ec.chain_rays(a, b, IDENT)
    S = SURF if surf else None
    A, Bk, U = (vc.Brick(x, t, rate) for x in (a, b, u))
    first = sc.march(A, S, r, IDENT)
    go, on = ec.hop(first)
    second = first.copy()
    second[go] = sc.march(Bk, S, on, IDENT)
    want = sc.march(U, S, r, IDENT)
    bits(second, want, ("color", "w", "t_min", "t", "depth"))
    both = (first["t_min"] != r["t_min"]) & (second["t_min"] != first["t_min"])
    assert both.sum() >= 200 and (want["w"] > 0).sum() >= 200


@pytest.mark.parametrize("counts", [(2, 2, 2), (2, 9, 10), (17, 2, 2)])
def test_thin_volumes_split_into_one_cell_bricks(counts):
    """The thin volumes cut along their longest axis at vertex 1: a one-cell brick, then the rest (the whole again where one cell is all)."""
    vol = ec.thin(counts)
    t = tf("cool")
    ax = int(np.argmax(counts))
    r = ec.edge_rays(vol, IDENT)
    r = r[(np.nan_to_num(r["direction"][:, ax]) >= 0) & (r["w"] == 0)]
    with np.errstate(all="ignore"):
        whole = vc.march(vc.Brick(vol, t, 1.7), r, IDENT)
    assert (whole["w"] > 0).sum() >= 100
    if counts[ax] == 2:
        return
    ca, cb, ob = list(counts), list(counts), [0, 0, 0]
    ca[ax], cb[ax], ob[ax] = 2, counts[ax] - 1, 1
    with np.errstate(all="ignore"):
        first = vc.march(vc.Brick(ec.cut(vol, (0, 0, 0), ca), t, 1.7), r, IDENT)
        go, on = ec.hop(first)
        second = first.copy()
        second[go] = vc.march(vc.Brick(ec.cut(vol, ob, cb), t, 1.7), on, IDENT)
    bits(second, whole, ("color", "w", "t_min", "depth"))
