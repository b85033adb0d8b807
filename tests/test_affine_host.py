"""Instance matrices with rotation, shear and mirroring, on the host: the checker's matrix arithmetic against known answers from the
reference's own glm (tests/golden/ref_matrix_vectors.json), the oracle's Adapter::trace against a float64 world-space brute force for
every matrix family of tests/affine_cases.py, the world boxes of scenes.instance_bbox, and the numpy volume checkers under the same
families (bricked frames against the one-brick frame, the rigid-motion claim of lit volumes)."""
import json
import os

import numpy as np
import pytest

from gravit_amd import scenes
from gravit_amd.layouts import RAY_DTYPE, RAY_EPSILON, point_light
from oracle import orc
from tests import affine_cases as ac
from tests import volume_checker as vc
from tests.conftest import GOLDEN

F = np.float32
FLT_MAX = np.finfo(F).max


@pytest.fixture(scope="module")
def glm_vectors():
    return json.load(open(os.path.join(GOLDEN, "ref_matrix_vectors.json")))


def f32(words):
    return np.array(words, np.uint32).view(F)


def same_floats(a, b):
    """Bit for bit; a NaN equals any NaN (which NaN an operation returns is the processor's choice, not glm's)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


PRODUCTS = ((0, "point", "m"), (1, "vector", "m"), (0, "inv_point", "inverse"), (1, "inv_vector", "inverse"), (2, "mat3", "normal_matrix"))


# ------------------------------------------------------------------ glm's products and inverses
@pytest.mark.parametrize("family", ac.FAMILIES)
def test_matrix_products_equal_glm(glm_vectors, family):
    """mat4 * vec4(p, 1), mat4 * vec4(d, 0) and mat3 * vec3 of the reference's glm, recorded for full matrices (and their glm inverses) with
    zero, -0, inf and NaN components: the oracle's xfm_point / xfm_vector / mat3_mul and the numpy checkers' xfm_point / xfm_vector give the
    same bits.  A transposed block, a transposed normi or another parenthesisation fails here for every family but diag."""
    rows = glm_vectors[family]
    assert len(rows) * len(rows[0]["v"]) >= 36
    for row in rows:
        v = np.array([f32(x) for x in row["v"]])
        for kind, name, mat in PRODUCTS:
            want = np.array([f32(x) for x in row[name]])
            assert same_floats(orc.matrix_probe(kind, f32(row[mat]), v), want), (family, name)
            if kind < 2:
                with np.errstate(all="ignore"):
                    got = (vc.xfm_point, vc.xfm_vector)[kind](f32(row[mat]), v)
                assert same_floats(got, want), (family, name, "numpy checker")


def test_the_recorded_products_tell_a_transposed_matrix_and_another_order():
    """The fixture can see what a diagonal block cannot: on the rot vectors a transposed 3x3 block, a transposed normi and a left-to-right
    sum of mat4 * vec4 each change recorded bits."""
    rows = json.load(open(os.path.join(GOLDEN, "ref_matrix_vectors.json")))["rot"]
    t_block = t_normi = order = 0
    for row in rows:
        v = np.array([f32(x) for x in row["v"]])[:5]
        m, nm = f32(row["m"]), f32(row["normal_matrix"])
        mt = m.reshape(4, 4).copy()
        mt[:3, :3] = mt[:3, :3].T
        t_block += not same_floats(orc.matrix_probe(0, mt.reshape(16), v), np.array([f32(x) for x in row["point"]])[:5])
        t_normi += not same_floats(orc.matrix_probe(2, nm.reshape(3, 3).T.reshape(9), v), np.array([f32(x) for x in row["mat3"]])[:5])
        ltr = np.stack([((m[r] * v[:, 0] + m[4 + r] * v[:, 1]) + m[8 + r] * v[:, 2]) + m[12 + r] for r in range(3)], axis=1).astype(F)
        order += not same_floats(ltr, np.array([f32(x) for x in row["point"]])[:5])
    assert t_block == len(rows) and t_normi == len(rows) and order > 0


INVERSE_MEASURED = 1.503e-7  # the largest difference found on the recorded vectors (a shear matrix), relative to the largest entry of glm's result


def test_inverses_are_close_to_glm(glm_vectors):
    """scenes.instance_matrices inverts in float64 and rounds once; glm::inverse(mat4) and transpose(inverse(mat3(m))) (api.cpp:307-308)
    work in float32 cofactors, so the bits differ.  Measured on the 24 recorded matrices, largest |difference| relative to the largest
    entry of glm's result: diag 1.19e-7, mirror 1.24e-7, perm 7.5e-9, rot 9.3e-8, rot_scale 1.20e-7, shear 1.50e-7 (about one float32
    ulp: float64-then-round is the more accurate of the two).  Asserted: twice the largest.  The diag vectors differ too -- the matrices
    of today's scenes have never been glm's float32 bits; only three of the four perm vectors are equal."""
    worst = 0.0
    for family, rows in glm_vectors.items():
        for row in rows:
            minv, normi = scenes.instance_matrices(f32(row["m"]))
            for got, want in ((minv, f32(row["inverse"])), (normi, f32(row["normal_matrix"]))):
                worst = max(worst, float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()))
    print("largest relative difference to glm's inverses: %.4g" % worst)
    assert worst <= 2 * INVERSE_MEASURED


# ------------------------------------------------------------------ the oracle's Adapter::trace against the world-space brute force
def trace_rays(m, v, t, n, seed):
    org, d = ac.centroid_rays(m, v, t, n, seed)
    rays = np.zeros(n, RAY_DTYPE)
    rays["origin"], rays["direction"] = org, d
    rays["t_min"], rays["t_max"], rays["t"] = RAY_EPSILON, FLT_MAX, FLT_MAX
    rays["depth"], rays["w"], rays["id"] = 1, 1.0, np.arange(n)
    return rays


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("family", ac.FAMILIES)
def test_oracle_trace_equals_the_world_space_brute_force(family, seed):
    """orc.Mesh.trace under a full matrix (the ray taken into object space by minv) against float64 Moeller-Trumbore on the triangles
    taken into WORLD space by m -- a reference that knows nothing of minv, normi or their storage: 400 vertices / 900 triangles, 4,000
    rays aimed near triangle centroids from 4 units away.  Hit / miss agrees for every ray, the median relative error of t is below
    1e-6 and at most 1 % of the rays are above 1e-4 (grazing hits on large slivers)."""
    v, t = ac.random_mesh(seed)
    m = ac.matrix(family, seed)
    minv, normi = scenes.instance_matrices(m)
    rays = trace_rays(m, v, t, 4000, seed)
    orc.Mesh(v, t).trace(rays, m, minv, normi, point_light((5.0, 6.0, 7.0)), 0)
    t64 = ac.world_hits64(m, v, t, rays["origin"], rays["direction"], float(RAY_EPSILON))
    wrong, median, share = ac.check_against_world(rays["t"], t64)
    print("%s seed %d: %d hit/miss disagreements, median rel %.3g, share above 1e-4 %.4f, %d hits" % (family, seed, wrong, median, share, np.isfinite(t64).sum()))
    assert np.isfinite(t64).sum() > 2000
    assert wrong == 0 and median < 1e-6 and share <= 0.01


# ------------------------------------------------------------------ world boxes
def two_corner_box(m16, lo, hi):
    """The reference's rule (api.cpp:309-312), as scenes.instance_bbox stated it before: Box3D(M * min, M * max)."""
    M = m16.reshape(4, 4).T
    a = (M @ np.array([lo[0], lo[1], lo[2], 1], F)).astype(F)[:3]
    b = (M @ np.array([hi[0], hi[1], hi[2], 1], F)).astype(F)[:3]
    return np.minimum(a, b), np.maximum(a, b)


def existing_scenes():
    yield scenes.simple_scene(16, 16)
    yield scenes.bunny_scene(16, 16)
    yield scenes.bunny70k_scene(16, 16)
    yield scenes.bunny_grid_scene(4, 2, 0.3, 16, 16)
    yield scenes.soup_scene(2000, 16, 16)
    one = scenes.cathedral_scene(16, 16)
    yield one
    yield scenes.split_into_domains(one, 4)
    yield scenes.soup_domains_scene(4000, 8, 16, 16)
    yield scenes.soup_weak_scene(500, 4, 16, 16)
    yield scenes.load_conf(os.path.join(GOLDEN, "bunny.conf"), width=16, height=16)


def test_instance_boxes_of_every_existing_scene_are_unchanged():
    """Eight corners instead of two changes nothing that exists: for every instance of every scene builder, for the volume tests'
    matrices and for the diag family, scenes.instance_bbox equals the two-corner rule (np.array_equal), and the scene holds that box."""
    n = 0
    for sc in existing_scenes():
        for i in range(sc.n_inst):
            lo, hi = sc.meshes[sc.inst_mesh[i]].bbox()
            want = two_corner_box(sc.m[i], lo, hi)
            got = scenes.instance_bbox(sc.m[i], lo, hi)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (sc.name, i)
            assert np.array_equal(sc.inst_lo[i], want[0]) and np.array_equal(sc.inst_hi[i], want[1]), (sc.name, i)
            n += 1
    assert n > 50
    rng = np.random.default_rng(4)
    mats = [ac.matrix("diag", s) for s in range(40)] + [scenes.mat_translate_scale((0.3, -0.2, 0.5), (1.5, 1.5, 1.5)), scenes.mat_translate_scale((0, 0, 0), (1, 1, 1)),
                                                        scenes.mat_translate_scale((1, -2, 3), (-0.5, 2.0, -1.0))]
    for m in mats:
        lo = rng.normal(size=3).astype(F)
        hi = (lo + rng.uniform(0, 2, 3)).astype(F)
        want, got = two_corner_box(m, lo, hi), scenes.instance_bbox(m, lo, hi)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("family", ["rot", "rot_scale", "shear", "mirror", "perm"])
def test_instance_boxes_contain_the_instance(family):
    """Under a rotation the two-corner box does not contain the transformed vertices (the top level would cull rays that hit); the box
    of eight corners does, up to the rounding of one float32 product (2^-21 of the extent).  Under a signed axis permutation the two
    rules agree exactly."""
    v, t = ac.random_mesh(5)
    lo, hi = scenes.MeshData(v, t).bbox()
    for seed in range(6):
        m = ac.matrix(family, seed)
        M = m.reshape(4, 4).T.astype(np.float64)
        w = v.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
        old, new = two_corner_box(m, lo, hi), scenes.instance_bbox(m, lo, hi)
        slack = 2.0 ** -21 * float(np.abs(w).max())
        assert (w >= new[0] - slack).all() and (w <= new[1] + slack).all()
        if family == "perm":
            assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1])
        elif family == "rot":
            assert ((w < old[0] - slack) | (w > old[1] + slack)).any(), seed


# ------------------------------------------------------------------ volumes: the numpy frame loop under the families
def test_checker_frames_under_an_axis_permutation_do_not_depend_on_the_bricking():
    """volume_checker.frame with the eight-corner world boxes: under a signed, scaled axis permutation, with and without mirroring (and
    under a diagonal matrix) a brick's world box is the brick, and 8 and 27 bricks give the one-brick framebuffer in every bit."""
    from tests import volume_affine_cases as va
    for name in ("perm", "perm_mirror", "diag"):
        one = va.frame_reference(name, (1, 1, 1))[0]
        assert (one[..., 3] > 0).sum() > 500
        for split in va.SPLITS[1:]:
            assert np.array_equal(va.frame_reference(name, split)[0].view(np.uint32), one.view(np.uint32)), (name, split)


def test_checker_frames_of_turned_bricks_lose_samples_so_the_tracers_refuse_them():
    """The same under a rotation, rotation x scale, a shear, a mirrored rotation: the world boxes of neighbouring bricks overlap, and
    next_brick's rule (a brick is entered only if its exit lies strictly beyond the last brick's) skips bricks.  Measured here on the 64 x 48
    film, pixels that differ from the one-brick frame (largest difference): rot@1 33 / 36 of 934 lit (0.16), rot@2 62 / 94 of 932 (0.996),
    shear 13 / 19 of 302 (0.996), rot_scale 6 / 11 of 475 (0.115), mirror 11 / 18 of 432 (0.995) for 8 / 27 bricks; rot (seed 0) happens
    to lose none.  So 8 and 27 bricks do NOT reproduce one brick, and the multi-brick tracers refuse such a matrix (before any device
    object is made: the refusal needs no GPU); one brick, and any matrix that keeps the axes parallel, are taken."""
    from gravit_amd.scheduler import HipVolumeBackend, VolumeTracer, axis_aligned_matrix
    from tests import volume_affine_cases as va
    from tests import volume_fused_cases as fc
    from tests.volume_common import tf
    lost = {}
    for name in ("rot@1", "rot@2", "shear", "rot_scale", "mirror"):
        one = va.frame_reference(name, (1, 1, 1))[0]
        for split in va.SPLITS[1:]:
            fb = va.frame_reference(name, split)[0]
            lost[name, split] = int((fb.view(np.uint32) != one.view(np.uint32)).any(axis=2).sum())
    print(lost)
    assert all(n > 0 for n in lost.values()), lost
    # the fused formulation (tests/volume_fused_checker.py: every ray followed to its end) applies the same rule and loses the same samples
    from gravit_amd.scheduler import _brick_boxes
    from tests import volume_fused_checker as fz
    for name in ("rot@1", "shear"):
        m = va.matrix(name)
        cut = fc.bricks_of(va.volume(), (2, 2, 2))
        lo, hi = _brick_boxes(cut, m)
        fused = fz.frame([vc.Brick(b, tf("cool"), va.RATE) for b in cut], lo, hi, scenes.instance_matrices(m)[0], va.camera(m))[0]
        assert np.array_equal(fused.view(np.uint32), va.frame_reference(name, (2, 2, 2))[0].view(np.uint32))
        assert not np.array_equal(fused.view(np.uint32), va.frame_reference(name, (1, 1, 1))[0].view(np.uint32))
    parts = fc.bricks_of(va.volume(), (2, 2, 2))
    for name in ("rot", "rot@1", "rot_scale", "shear", "mirror"):
        m = va.matrix(name)
        assert not axis_aligned_matrix(m)
        for cls in (VolumeTracer, HipVolumeBackend):
            with pytest.raises(ValueError, match="world boxes of neighbouring bricks overlap"):
                cls(parts, va.camera(m), tf("cool"), m=m, sampling_rate=va.RATE)
        # ... MixedTracer before its mesh tracer and depth plane exist, VolumeDomainTracer whatever backend it is given
        from gravit_amd.scheduler import MixedTracer, VolumeDomainTracer
        from tests.fake_dist import FakeWorld
        with pytest.raises(ValueError, match="MixedTracer: 8 bricks"):
            MixedTracer(scenes.simple_scene(16, 16), parts, va.camera(m), tf("cool"), m=m, sampling_rate=va.RATE)
        with pytest.raises(ValueError, match="VolumeDomainTracer: 8 bricks"):
            VolumeDomainTracer(parts, [0] * 8, va.camera(m), tf("cool"), FakeWorld(1).rank_view(0), None, "cpu", m=m, sampling_rate=va.RATE, backend=object())
    for name in ("perm", "perm_mirror", "diag", "ident"):
        assert axis_aligned_matrix(va.matrix(name))


def test_lit_fog_turned_with_its_lights_and_camera_on_the_checker():
    """The measurement behind tests/test_gpu_volume_affine.py's rigid-motion bound: volume_shade_checker.frame of the lit one-brick fog under
    a rotation, the camera and the lights turned with it, against the unrotated frame.  Largest per-channel difference: rot 1.62e-6,
    rot@1 2.15e-6, rot@2 1.07e-6, rot@3 2.44e-6; no pixel above 1e-5 in any of them (932 lit pixels).  The GPU test uses rot and rot@1
    and asserts four times their larger value.  Under a shear the same construction is another picture (0.99, 30 % of the film): object-space
    lighting equals world-space lighting for rigid motions and uniform scales only."""
    from tests import volume_affine_cases as va
    base = va.lit_frame_reference("ident")
    assert (base[..., 3] > 0).sum() > 500
    worst = 0.0
    for name in ("rot", "rot@1"):
        largest, share = va.frame_difference(va.lit_frame_reference(name), base)
        print(name, largest, share)
        worst = max(worst, largest)
        assert share == 0.0
    assert 0.5 * va.RIGID_MEASURED < worst <= 1.001 * va.RIGID_MEASURED  # the recorded value is the measured one
    largest, share = va.frame_difference(va.lit_frame_reference("shear"), base)
    assert largest > 0.1 and share > 0.05
