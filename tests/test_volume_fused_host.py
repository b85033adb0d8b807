"""The fused frame, host side (no GPU): the per-ray formulation (tests/volume_fused_checker.py: every ray followed to its end, no queues)
gives the frame loop's bits (tests/volume_checker.frame, tests/volume_clip_checker.frame) and the same number of (ray, brick) visits on
the brickings the device test uses -- so that test's reference is not the code under test.  Also: the header and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gravit_amd import capi, scenes
from tests import volume_checker as vc
from tests import volume_fused_cases as fc
from tests import volume_fused_checker as fz
from tests.conftest import ROOT
from tests.test_gpu_volume import tf

F = np.float32


def test_header_declares_and_binding_lists_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "gvt_hip.h")).read()
    assert re.search(r"\bgvt_hip_volume_frame_fused\s*\(", hdr) and "gvt_hip_volume_frame_fused" in capi.SYMBOLS
    assert int(re.search(r"#define GVT_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 6  # additive: the revision stays
    body = re.search(r"typedef struct \{([^}]*)\} gvt_hip_volume_fused_stats;", hdr).group(1)
    names = re.findall(r"\b(?:uint32_t|uint64_t)\s+(\w+);", body)
    assert names == [k for k, _ in capi.VolumeFusedStats._fields_]
    assert C.sizeof(capi.VolumeFusedStats) == 8 + 5 * 8


def fused(split, table, moved, where):
    parts = fc.bricks_of(fc.volume(), split)
    m = fc.matrix(moved)
    lo, hi = fc.world_boxes(parts, m)
    return fz.frame([vc.Brick(b, tf(table), fc.RATE) for b in parts], lo, hi, scenes.instance_matrices(m)[0], fc.camera(where, moved))


@pytest.mark.parametrize("split", fc.SPLITS)
@pytest.mark.parametrize("table,moved,where", [("cool", False, "outside"), ("opaque", True, "inside"), ("spikes", True, "outside")])
def test_per_ray_formulation_gives_the_loops_bits_and_visits(split, table, moved, where):
    want, rounds, entering = fc.reference(split, table, moved, where)
    got, counters = fused(split, table, moved, where)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert (want[..., 3] > 0).sum() > (0 if table == "spikes" else 200)  # the volume shows (the sparse table leaves most of this small grid transparent)
    assert counters["brick_visits"] == sum(n for _, n in rounds)
    assert counters["rays_deposited"] == entering > 200
    if split != (1, 1, 1) and table != "opaque":  # (the opaque table ends every ray in its first brick)
        assert counters["brick_visits"] > entering  # rays go on from brick to brick


def test_the_cut_does_not_show():
    frames = [fc.reference(s, "cool", True, "inside")[0] for s in fc.SPLITS]
    for f in frames[1:]:
        assert (f.view(np.uint32) == frames[0].view(np.uint32)).all()


@pytest.mark.parametrize("split", [(2, 2, 2), (4, 4, 4)])
def test_per_ray_formulation_under_a_depth_plane(split):
    want, plane = fc.clip_reference(split, "cool", False)
    parts = fc.bricks_of(fc.volume(), split)
    lo, hi = fc.world_boxes(parts, fc.matrix(False))
    got, counters = fz.frame([vc.Brick(b, tf("cool"), fc.RATE) for b in parts], lo, hi, scenes.instance_matrices(fc.matrix(False))[0],
                             fc.camera("outside"), plane)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    plain = fc.reference(split, "cool", False, "outside")[0]
    assert (got[..., 3] < plain[..., 3]).sum() > 200  # the clip shows
    assert np.isinf(plane).sum() > 500 and np.isfinite(plane).sum() > 1500
    assert counters["rays_deposited"] > 200


def test_a_camera_looking_away_meets_no_brick():
    want, rounds, entering = fc.reference((2, 2, 2), "cool", False, "away")
    assert entering == 0 and not rounds and not want.any()
    got, counters = fused((2, 2, 2), "cool", False, "away")
    assert not got.any() and counters == {"brick_visits": 0, "rays_deposited": 0}
