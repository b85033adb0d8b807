"""Animated scenes, host side (no GPU): the new entry points are declared, bound and exported, and NativeTracer.update_scene refuses a scene
whose topology differs before it reaches the device."""
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import HipMeshAdapter, TopLevel
from gravit_amd.scheduler import NativeTracer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gvt_hip_mesh_update_vertices", "gvt_hip_top_update", "gvt_hip_tracer_set_transforms"]


def test_header_declares_the_animation_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gvt_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS
    assert re.search(r"#define\s+GVT_HIP_UPDATE_DEVICE\s+1u", hdr)


def test_library_exports_the_animation_entry_points():
    so = capi.LIB_PATH
    if not os.path.exists(so):
        pytest.fail("%s is missing: build() first" % so)
    exported = set(re.findall(r" T (gvt_hip_\w+)", subprocess.run(["nm", "-D", so], check=True, stdout=subprocess.PIPE, text=True).stdout))
    assert set(NEW) <= exported


def test_python_layer_has_the_animation_calls():
    assert callable(getattr(HipMeshAdapter, "update_vertices", None))
    assert callable(getattr(TopLevel, "update", None))
    assert callable(getattr(NativeTracer, "update_scene", None)) and callable(getattr(NativeTracer, "set_transforms", None))


def test_update_scene_refuses_a_topology_change():
    sc = scenes.bunny_grid_scene(nx=2, ny=1, width=32, height=32)
    fake = SimpleNamespace(scene=sc)
    fewer = scenes.bunny_grid_scene(nx=1, ny=1, width=32, height=32)
    with pytest.raises(ValueError, match="instance set"):
        NativeTracer.update_scene(fake, fewer)
    m = sc.meshes[0]
    tris = m.tris.copy()
    tris[0] = tris[0][::-1]
    other = scenes.Scene([scenes.MeshData(m.verts, tris, m.material)], sc.inst_mesh, sc.m, sc.minv, sc.normi, sc.inst_lo, sc.inst_hi, sc.lights,
                         sc.camera, sc.name)
    with pytest.raises(ValueError, match="topology"):
        NativeTracer.update_scene(fake, other)
    fewer_verts = scenes.Scene([scenes.MeshData(np.ascontiguousarray(m.verts[:-1]), m.tris, m.material)], sc.inst_mesh, sc.m, sc.minv, sc.normi,
                               sc.inst_lo, sc.inst_hi, sc.lights, sc.camera, sc.name)
    with pytest.raises(ValueError, match="topology"):
        NativeTracer.update_scene(fake, fewer_verts)
