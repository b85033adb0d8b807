"""Meshes shadowing the volume without a device: the cases' conditions (tests/volume_mesh_shadow_cases.py), the numpy checker
(tests/volume_mesh_shadow_checker.py) against the fog checker it restates, the properties of its frame, and the Python surface's
refusals."""
import numpy as np
import pytest

from gravit_amd import capi
from gravit_amd.scheduler import MixedTracer, VolumeDomainTracer, VolumeTracer
from tests import volume_fused_cases as fc
from tests import volume_mesh_shadow_cases as mc
from tests import volume_mesh_shadow_checker as mg

F = np.float32
WHERE = "inside"
SPLIT = (2, 2, 2)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("moved", [False, True])
def test_the_scene_shadows_some_cells_wholly_and_some_in_part(moved):
    """The issue's conditions, for both lights: blocked share of the vertices in [0.10, 0.50], cells with mixed corners >= 0.05 of the
    cells, cells with all eight corners blocked >= 0.05.  The third instance blocks nothing."""
    O, usable, blocked = mc.occluder_grid(moved)
    assert usable.all() and O.shape == (2, fc.N, fc.N, fc.N) and O.dtype == np.uint8 and set(np.unique(O)) == {0, 1}
    assert blocked == int((O == 0).sum())
    for j in range(2):
        share, mixed, full = mc.cell_shares(O[j])
        print("moved %d light %d: blocked %.3f mixed %.3f all blocked %.3f" % (moved, j, share, mixed, full))
        assert 0.10 <= share <= 0.50 and mixed >= 0.05 and full >= 0.05, (share, mixed, full)
    scene = mc.scene(moved)
    assert scene.n_inst == 3 and len(scene.meshes[0].tris) == 80 and len(scene.meshes[1].tris) == 2
    B, _, _, m, _, S, _ = mc.whole("lit", moved)
    alone = mg.occluders(B, m, type(scene)(scene.meshes, [1], scene.m[2:], scene.minv[2:], scene.normi[2:], scene.inst_lo[2:], scene.inst_hi[2:], scene.lights,
                                           scene.camera), S)
    assert alone[2] == 0 and (alone[0] == 1).all()
    assert not np.allclose(scene.m[0].reshape(4, 4)[:3, :3], np.diag(np.diag(scene.m[0].reshape(4, 4)[:3, :3])))  # rotation and shear


def test_no_mesh_and_a_wall():
    none, _, n_none = mc.occluder_grid(False, "none")
    wall, _, n_wall = mc.occluder_grid(False, "wall")
    assert (none == 1).all() and n_none == 0
    assert (wall == 0).all() and n_wall == 2 * fc.N ** 3
    shifted = mc.occluder_grid(False, "shifted")[0]
    assert (shifted != mc.occluder_grid(False)[0]).any()


@pytest.mark.parametrize("mode", mc.MODES)
def test_with_every_vertex_clear_the_frame_is_the_fog_checkers(mode):
    """O = 1 everywhere: volume_fog_shadow_checker.frame in every bit, and the counters."""
    got, counters, _ = mc.reference(mode, SPLIT, WHERE, which="none")
    want, wc = mc.fog_reference(mode, SPLIT, WHERE)
    assert (bits(got) == bits(want)).all() and got.any()
    for key in wc:
        if key != "shaded_pixels":
            assert counters[key] == wc[key], key


@pytest.mark.parametrize("mode", mc.MODES)
def test_with_every_vertex_blocked_the_frame_is_the_unlit_one(mode):
    """O = 0 everywhere: the bits of the same frame rendered with kd = 0."""
    got, _, _ = mc.reference(mode, SPLIT, WHERE, which="wall")
    want, _ = mc.fog_reference(mode, SPLIT, WHERE, kd=0.0)
    assert (bits(got) == bits(want)).all() and got.any()


@pytest.mark.parametrize("mode", mc.MODES)
def test_the_shadows_show(mode):
    """With the case's O the frame differs from the fog checker's on at least 200 pixels (a condition of the case), never in opacity,
    never brighter; no counter moves."""
    got, counters, _ = mc.reference(mode, SPLIT, WHERE)
    plain, pc = mc.fog_reference(mode, SPLIT, WHERE)
    differ = (bits(got) != bits(plain)).any(axis=-1)
    print("%s: %d of %d pixels differ" % (mode, differ.sum(), differ.size))
    assert differ.sum() >= 200
    assert (bits(got[..., 3]) == bits(plain[..., 3])).all() and (got[..., :3] <= plain[..., :3]).all()
    for key in pc:
        if key != "shaded_pixels":
            assert counters[key] == pc[key], key


@pytest.mark.parametrize("mode", mc.MODES)
def test_the_brickings_agree(mode):
    frames = [mc.reference(mode, s, WHERE)[0] for s in [(1, 1, 1), (2, 2, 2), (4, 4, 4)]]
    for f in frames[1:]:
        assert (bits(f) == bits(frames[0])).all()


def test_the_binding_names_the_entry_points():
    for name in ("gvt_hip_volume_occluder_grid_bake", "gvt_hip_volume_occluder_grid_download", "gvt_hip_volume_occluder_grid_info",
                 "gvt_hip_volume_occluder_grid_release", "gvt_hip_volume_frame_mesh_shadowed"):
        assert name in capi.SYMBOLS
    assert [n for n, _ in capi.VolumeOccluderStats._fields_][:4] == ["rays", "rays_blocked", "any_hit_launches", "bytes"]
    assert [n for n, _ in capi.VolumeMeshShadowStats._fields_] == ["fog", "mesh_shadowed", "pad"]


def test_mesh_shadows_need_fog_shadows_and_one_device():
    with pytest.raises(ValueError, match="mesh_shadows"):
        VolumeTracer([], None, None, mesh_shadows=True)
    with pytest.raises(ValueError, match="mesh_shadows"):
        VolumeTracer([], None, None, shadows=True, mesh_shadows=True)
    with pytest.raises(ValueError, match="mesh_shadows"):
        VolumeDomainTracer([], [], None, None, None, None, None, mesh_shadows=True)
    assert "mesh_shadows" in MixedTracer.__init__.__code__.co_varnames
