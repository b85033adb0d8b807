"""Shadowed surfaces, host side (no GPU): the numpy checker (tests/volume_shadow_checker.py) has the properties the contract states --
the same bits for every bricking, the unshadowed frame's bits where no shadow falls, the kd = 0 frame's bits where every light is
blocked -- and the cases (tests/volume_shadow_cases.py) exercise shadow rays of both kinds.  Also: the header and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gravit_amd import capi
from tests import volume_fused_cases as fc
from tests import volume_shadow_cases as swc
from tests.conftest import ROOT

F = np.float32
N_PIX = fc.FILM[0] * fc.FILM[1]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_header_binding_and_abi_agree():
    hdr = open(os.path.join(ROOT, "include", "gvt_hip.h")).read()
    assert re.search(r"\bgvt_hip_volume_frame_shadowed\s*\(", hdr) and "gvt_hip_volume_frame_shadowed" in capi.SYMBOLS
    assert int(re.search(r"#define GVT_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 6 == capi.ABI_VERSION  # additive: the revision stays

    def names(struct):
        body = re.search(r"typedef struct \{((?:[^}]|\n)*?)\} %s;" % struct, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in re.findall(r"\b(?:uint32_t|int32_t|uint64_t)\s+([\w\s,]+);", body):
            out += [n.strip() for n in decl.split(",")]
        return out

    assert names("gvt_hip_volume_shadow_params") == [k for k, _ in capi.VolumeShadowParams._fields_]
    assert names("gvt_hip_volume_shadow_stats") == [k for k, _ in capi.VolumeShadowStats._fields_]
    assert names("gvt_hip_volume_shadow_stats")[:9] == names("gvt_hip_volume_fused_shaded_stats")  # same fields, same order
    assert C.sizeof(capi.VolumeShadowParams) == 8
    assert C.sizeof(capi.VolumeShadowStats) == C.sizeof(capi.VolumeFusedShadedStats) + 8 + 5 * 8 == 112
    assert capi.VolumeShadowStats.shadowed.offset == C.sizeof(capi.VolumeFusedShadedStats) and capi.VolumeShadowStats.shadow_rays.offset == 72


@pytest.mark.parametrize("where", sorted(swc.CAMERAS))
def test_the_cut_does_not_show(where):
    frames = [swc.reference("main", s, where) for s in fc.SPLITS]
    for fb, counters, _, _ in frames[1:]:
        assert (bits(fb) == bits(frames[0][0])).all()
        assert counters["shadow_rays"] == frames[0][1]["shadow_rays"] and counters["shadow_crossings"] == frames[0][1]["shadow_crossings"]
    assert frames[0][0].any()
    visits = [c["shadow_brick_visits"] for _, c, _, _ in frames]
    assert visits[3] > visits[1] > visits[0]  # shadow rays go from brick to brick


def test_main_case_has_shadow_rays_of_both_kinds():
    """At least a tenth of the shadow rays meet nothing (A_s == 0) and at least a tenth meet something (A_s > 0) -- at the outside eye;
    at the inside eye every shadow ray starts deep in table "cool"'s fog, so all of its A_s are > 0 (the cases file records the shares)."""
    fb, counters, details, _ = swc.reference("main", (1, 1, 1), "outside")
    A_s = details["A_s"][:, details["usable"]].reshape(-1)
    assert len(A_s) == counters["shadow_rays"] >= 500
    assert (A_s == 0).mean() >= 0.1 and (A_s > 0).mean() >= 0.1
    plain = swc.unshadowed("main", (1, 1, 1), "outside")[0]
    assert (bits(fb) != bits(plain)).any(axis=-1).sum() >= 100  # the shadows show
    assert (bits(fb)[..., 3] == bits(plain)[..., 3]).all()  # ... in the colour alone: opacity does not depend on it


@pytest.mark.parametrize("split", [(1, 1, 1), (2, 2, 2)])
def test_identity_case_has_the_unshadowed_bits(split):
    fb, counters, details, _ = swc.reference("identity", split, "outside", moved=False)
    plain, pc = swc.unshadowed("identity", split, "outside", moved=False)
    assert counters["shadow_rays"] > 500 and counters["shadow_crossings"] == 0 and not details["A_s"].any()
    assert (bits(fb) == bits(plain)).all()
    for key in pc:
        assert counters[key] == pc[key], key
    assert fb.any()


@pytest.mark.parametrize("split", [(1, 1, 1), (2, 2, 2)])
def test_occluder_case_has_the_ambient_bits_where_every_light_is_blocked(split):
    fb, counters, details, _ = swc.reference("occluder", split, "outside", moved=False)
    ambient = swc.unshadowed("occluder", split, "outside", kd=0.0, moved=False)[0]
    plain = swc.unshadowed("occluder", split, "outside", moved=False)[0]
    has, dark = swc.fully_shadowed(details, N_PIX)
    assert has.sum() > 500 and dark.sum() >= 0.5 * has.sum()
    got, amb, pl = bits(fb).reshape(-1, 4), bits(ambient).reshape(-1, 4), bits(plain).reshape(-1, 4)
    assert (got[dark] == amb[dark]).all()
    assert (got[dark] != pl[dark]).any(axis=-1).all()  # the light would have shown there
    lit = has & ~dark
    assert lit.any() and (got[lit] == pl[lit]).all()  # here T is 0 or 1: a pixel not in the shadow is fully lit


def test_bias_shows():
    one = swc.reference("main", (1, 1, 1), "outside", bias=1)
    two = swc.reference("main", (1, 1, 1), "outside", bias=2)
    assert (bits(one[0]) != bits(two[0])).any()
    assert one[1]["shadow_rays"] == two[1]["shadow_rays"]  # the camera rays' samples do not depend on it


def test_domain_tracer_refuses_shadows():
    """A rank does not hold the foreign bricks a shadow ray needs: out of scope, and said so before anything is built."""
    from gravit_amd.scheduler import VolumeDomainTracer

    with pytest.raises(ValueError, match="shadows"):
        VolumeDomainTracer([], [], None, None, None, None, None, shadows=True)
