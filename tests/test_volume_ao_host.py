"""The ambient occlusion checker (tests/volume_ao_checker.py) pinned on the host, without a device: the ownership walk gives the one
brick's bits in every bricking, axis-parallel directions included; radius = dt gives the grid of ones; the cases of
tests/volume_ao_cases.py are not vacuous; with a grid of ones the checker's frame is the fog-shadowed checker's in every bit, with
ka = 0 it is the base frame's at ka = 0, and with the case's grid it moves pixels."""
import numpy as np
import pytest

from tests import volume_ao_cases as aoc
from tests import volume_ao_checker as ao
from tests import volume_checker as vc
from tests import volume_fog_shadow_cases as fgc
from tests import volume_fused_cases as fc

F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def owned(mode, split, moved, which):
    B, _, _, m, minv, S, _ = fgc.whole(mode, moved)
    _, on, table = aoc.swc.surfaces("main", mode)
    bricks = [vc.Brick(b, table, fc.RATE) for b in fc.bricks_of(fc.volume(), split)]
    return ao.grid_owned(bricks, B, m, minv, S, aoc.dirs(which), aoc.radius(), aoc.GRID_BIAS)


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("split", fc.SPLITS)
@pytest.mark.parametrize("mode", aoc.MODES)
def test_the_ownership_walk_gives_the_one_bricks_bits(mode, split, moved):
    want, _ = aoc.ao_grid(mode, moved)
    assert (bits(owned(mode, split, moved, "main")) == bits(want)).all()


@pytest.mark.parametrize("split", fc.SPLITS)
@pytest.mark.parametrize("mode", aoc.MODES)
def test_directions_that_run_in_brick_faces(mode, split):
    want, _ = aoc.ao_grid(mode, False, "parallel")
    assert (bits(owned(mode, split, False, "parallel")) == bits(want)).all()
    assert ((want > 0) & (want < 1)).mean() > 0.5


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("mode", aoc.MODES)
def test_radius_dt_gives_all_ones_and_the_cases_are_not_vacuous(mode, moved):
    assert (aoc.ao_grid(mode, moved, "main", 1.0)[0] == F(1)).all()
    assert not (aoc.ao_grid(mode, moved, "main", 1.5)[0] == F(1)).all()  # (one more half step and the grid is no longer the trivial one)
    AO, crossings = aoc.ao_grid(mode, moved)
    share = float(((AO > 0) & (AO < 1)).mean())
    print("%s moved=%d: share of vertices with 0 < AO < 1 = %.3f, crossings %d" % (mode, moved, share, crossings))
    assert share >= 0.5
    assert (crossings > 0) == (mode == "surf_lit")
    assert (AO >= 0).all() and (AO <= 1).all()


@pytest.mark.parametrize("where", sorted(aoc.CAMERAS))
@pytest.mark.parametrize("mode", aoc.MODES)
def test_a_grid_of_ones_gives_the_fog_shadowed_checkers_frame(mode, where):
    got, counters, _ = aoc.reference(mode, (2, 2, 2), where, grid="ones")
    want, base_counters, _ = fgc.reference(mode, (2, 2, 2), where)
    assert (bits(got) == bits(want)).all() and want.any()
    for key in counters:
        assert counters[key] == base_counters[key], key


@pytest.mark.parametrize("mode", aoc.MODES)
def test_without_ambient_light_the_frame_is_the_base_frame(mode):
    got, _, _ = aoc.reference(mode, (2, 2, 2), "inside", ka=0.0)
    want, _ = aoc.base(mode, (2, 2, 2), "inside", ka=0.0)
    assert (bits(got) == bits(want)).all() and want.any()


@pytest.mark.parametrize("where", sorted(aoc.CAMERAS))
@pytest.mark.parametrize("mode", aoc.MODES)
def test_the_grid_moves_pixels_and_no_counter(mode, where):
    got, counters, _ = aoc.reference(mode, (2, 2, 2), where)
    want, base_counters = aoc.base(mode, (2, 2, 2), where)
    seen = want[..., 3] != 0
    moved = (bits(got) != bits(want)).any(axis=2) & seen
    print("%s %s: %d of %d pixels with alpha differ" % (mode, where, int(moved.sum()), int(seen.sum())))
    assert seen.sum() > 0 and moved.sum() >= 0.1 * seen.sum()
    assert (bits(got[..., 3]) == bits(want[..., 3])).all()  # (A never depends on AO)
    assert (got[..., :3] <= want[..., :3]).all()  # (AO <= 1 only darkens)
    for key in counters:
        assert counters[key] == base_counters[key], key
