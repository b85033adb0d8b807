"""The shaded fused frame, host side (no GPU): the per-ray formulation (tests/volume_fused_shaded_checker.py) gives the frame loop's bits
(tests/volume_shade_checker.frame) and its crossings and shaded counts for every case the device test uses -- so that test's reference
is not the code under test -- and the cases exercise the side mask a ray carries from brick to brick.  Also: the header and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gravit_amd import capi
from tests import volume_fused_cases as fc
from tests import volume_fused_shaded_cases as sh
from tests import volume_fused_shaded_checker as fs
from tests import volume_shade_checker as lc
from tests.conftest import ROOT

F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_header_declares_and_binding_lists_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "gvt_hip.h")).read()
    assert re.search(r"\bgvt_hip_volume_frame_fused_shaded\s*\(", hdr) and "gvt_hip_volume_frame_fused_shaded" in capi.SYMBOLS
    assert int(re.search(r"#define GVT_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 6  # additive: the revision stays
    body = re.search(r"typedef struct \{([^}]*)\} gvt_hip_volume_fused_shaded_stats;", hdr).group(1)
    names = []
    for decl in re.findall(r"\b(?:uint32_t|uint64_t)\s+([\w\s,]+);", body):
        names += [n.strip() for n in decl.split(",")]
    assert names == [k for k, _ in capi.VolumeFusedShadedStats._fields_]
    assert C.sizeof(capi.VolumeFusedShadedStats) == 8 + 7 * 8
    assert int(re.search(r"#define GVT_HIP_FUSED_SURFACES\s+(\d+)u", hdr).group(1)) == capi.FUSED_SURFACES == 1
    assert int(re.search(r"#define GVT_HIP_FUSED_LIT\s+(\d+)u", hdr).group(1)) == capi.FUSED_LIT == 2


@pytest.mark.parametrize("where", sorted(sh.CAMERAS))
@pytest.mark.parametrize("split", fc.SPLITS)
@pytest.mark.parametrize("mode", sorted(sh.MODES))
def test_per_ray_formulation_gives_the_loops_bits_and_counts(mode, split, where):
    bricks, lo, hi, minv, cam, S, shading, _ = sh.setup(split, mode, where)
    want, calls = lc.frame(bricks, lo, hi, minv, cam, S, shading)
    shaded = lc.frame.shaded
    again, loop = sh.loop_frame(bricks, lo, hi, minv, cam, S, shading)
    assert (bits(again) == bits(want)).all() and loop["samples_shaded"] == shaded and loop["adapter_calls"] == calls  # (the restated loop is the loop)
    got, counters, _ = sh.reference(split, mode, where)
    assert (bits(got) == bits(want)).all()
    assert (want[..., 3] > 0).sum() > 200  # the volume shows
    assert counters["crossings_rendered"] == loop["crossings_rendered"] and counters["samples_shaded"] == loop["samples_shaded"]
    if mode != "lit":
        assert counters["crossings_rendered"] > 0
    else:
        assert counters["crossings_rendered"] == 0
    if mode != "surf":
        assert counters["samples_shaded"] > 0
    else:
        assert counters["samples_shaded"] == 0
    if split != (1, 1, 1):
        assert counters["brick_visits"] > counters["rays_deposited"] > 200  # rays go on from brick to brick


@pytest.mark.parametrize("split", [(2, 2, 2), (4, 4, 4)])
@pytest.mark.parametrize("mode", sorted(sh.MODES))
def test_per_ray_formulation_under_a_depth_plane(mode, split):
    bricks, lo, hi, minv, cam, S, shading, _ = sh.setup(split, mode, "outside", False)
    got, counters, plane = sh.reference(split, mode, "outside", True)
    want, _ = lc.frame(bricks, lo, hi, minv, cam, S, shading, plane)
    assert (bits(got) == bits(want)).all()
    free, _ = lc.frame(bricks, lo, hi, minv, cam, S, shading)
    assert (got[..., 3] < free[..., 3]).any()  # the clip shows
    assert counters["rays_deposited"] > 200


@pytest.mark.parametrize("split", sh.MULTI)
@pytest.mark.parametrize("mode", ["surf", "surf_lit"])
def test_the_cases_need_the_carried_side_mask(mode, split):
    """A checker that drops GVT_HIP_RAY_SIDES between two visits (so the first sample of every visit has no previous sides) differs
    from the right one in at least 500 of the 3,072 pixels at the inside camera."""
    bricks, lo, hi, minv, cam, S, shading, _ = sh.setup(split, mode, "inside")
    right = sh.reference(split, mode, "inside")[0]
    wrong, _ = fs.frame(bricks, lo, hi, minv, cam, S, shading, keep_sides=False)
    assert (bits(wrong) != bits(right)).any(axis=-1).sum() >= 500


@pytest.mark.parametrize("mode", sorted(sh.MODES))
def test_the_cut_does_not_show(mode):
    frames = [sh.reference(s, mode, "inside")[0] for s in fc.SPLITS]
    for f in frames[1:]:
        assert (bits(f) == bits(frames[0])).all()
