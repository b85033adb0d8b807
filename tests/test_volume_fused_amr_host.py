"""The fused AMR frame without a device: the per-ray checker (tests/volume_fused_amr_checker.py) gives the loop checkers' bits and the
same number of (ray, brick) visits on the scene of the GPU tests, in every mode, with and without a depth plane; the conditions on the
inputs that tests/test_gpu_volume_fused_amr.py relies on; and the allow bit's value in the binding and the header."""
import os
import re

import numpy as np
import pytest

from gravit_amd import capi
from tests import volume_amr_checker as ac
from tests import volume_amr_surface_checker as asc
from tests import volume_fused_amr_cases as fc
from tests.volume_common import IDENT


def loop_frame(mode, bricking, where, plane):
    """The loop's checker over the same bricks: (framebuffer, (ray, brick) visits = the sum of the rounds' queue sizes)."""
    cam = fc.camera(where)
    bricks, lo, hi = fc.checker_bricks(fc.parts_of(fc.scene(), bricking))
    S, shading = fc.checker_args(mode)
    rounds = []
    if S is None:
        fb, _ = ac.frame(bricks, lo, hi, IDENT, cam, plane, rounds=rounds)
    else:
        fb, _ = asc.frame(bricks, lo, hi, IDENT, cam, S, shading, plane, rounds=rounds)
    return fb, sum(n for _, n in rounds)


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("where", fc.EYES)
@pytest.mark.parametrize("bricking", fc.BRICKINGS)
@pytest.mark.parametrize("mode", sorted(fc.MODES))
def test_checker_gives_the_loop_checkers_bits_and_visits(mode, bricking, where, clipped):
    got, counts, plane = fc.reference(mode, bricking, where, clipped)
    want, visits = loop_frame(mode, bricking, where, plane)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert counts["brick_visits"] == visits > 0
    if clipped:
        full, _, _ = fc.reference(mode, bricking, where)
        assert (got.view(np.uint32) != full.view(np.uint32)).any()  # the plane cuts rays that would have gone on


@pytest.mark.parametrize("where", fc.EYES)
def test_the_frames_of_the_gpu_tests_cover_the_cases(where):
    """What the device tests need from the eight-brick frame, on the checker's counts.  Measured: outside 490 transitions plain -> AMR,
    773 AMR -> plain, 1322 refined samples, 5 crossings at level 2, 2141 lit pixels; inside 874 / 3072 / 16413 and 3072 lit pixels
    (its rays leave S0 through S0's own cells and S2's: no level-2 crossing is asked of it)."""
    fb, counts, _ = fc.reference("surf_lit", 8, where)
    print(where, counts, int((fb[..., 3] > 0).sum()))
    assert counts["plain_to_amr"] > 0 and counts["amr_to_plain"] > 0
    assert counts["samples_refined"] > 0
    assert counts["crossings"] > 0 and counts["shaded"] > 0 and counts["crossings_level"].get(1, 0) > 0
    if where == "outside":
        assert counts["crossings_level"].get(2, 0) > 0
    assert (fb[..., 3] > 0).sum() > 300
    one, c1, _ = fc.reference("surf_lit", 1, where)
    assert (one.view(np.uint32) == fb.view(np.uint32)).all()  # the cut does not show
    assert c1["samples_refined"] == counts["samples_refined"] and c1["crossings"] == counts["crossings"] and c1["shaded"] == counts["shaded"]
    assert c1["plain_to_amr"] == c1["amr_to_plain"] == 0
    parts = fc.parts_of(fc.scene(), 8)
    assert [i for i, b in enumerate(parts) if b.subgrids] == [0, 7]  # two of the eight bricks have subgrids


def test_the_allow_bit():
    assert capi.FUSED_AMR == 16
    assert capi.FUSED_AMR & (capi.FUSED_SURFACES | capi.FUSED_LIT | capi.FUSED_CENTRAL | 4) == 0
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gvt_hip.h")).read()
    m = re.search(r"^#define\s+GVT_HIP_FUSED_AMR\s+(\d+)u\b", header, re.M)
    assert m and int(m.group(1)) == capi.FUSED_AMR
    assert "gvt_hip_volume_frame_fused_amr" in capi.SYMBOLS
    fields = [k for k, _ in capi.VolumeFusedAmrStats._fields_]
    assert fields[:len(capi.VolumeFusedShadedStats._fields_)] == [k for k, _ in capi.VolumeFusedShadedStats._fields_]
    assert fields[-3:] == ["samples_refined", "amr_bricks", "pad"]
    import ctypes as C

    assert C.sizeof(capi.VolumeFusedAmrStats) == C.sizeof(capi.VolumeFusedShadedStats) + 16
