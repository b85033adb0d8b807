"""The scenes of tests/test_gpu_early_deposit.py and tests/test_early_deposit_host.py (knob early_deposit), each with the oracle's frame of it: rendered once, shared
between the two files, never written to.  The films are those of tests/test_gpu_xcd_stripes.py (the same soup, sizes and camera move), restated here: this module
imports no test module and nothing that needs a device."""
from dataclasses import replace

import numpy as np

from gravit_amd import scenes
from gravit_amd.layouts import NORMALS_FLAT, PHONG, default_material, point_light
from tests.helpers import oracle_render

N_TRIS, HALF = 3000, 0.04  # a soup dense enough that most camera rays that enter its box hit
FILMS = {
    "8x8": (8, 8, None),         # one tile
    "24x16": (24, 16, None),     # six tiles
    "72x40": (72, 40, None),     # nine tiles per row
    "200x120": (200, 120, 1.3),  # the camera moved sideways: the cube's box reaches past the film's left edge -- a partial rectangle, a compacted list, pixels no ray reaches
    "400x300": (400, 300, None),
    "800x600": (800, 600, None),  # side-lit, its any-hit launch holds more than share_min_rays = 131,072 shadow rays: the launch's drain shares rays between lanes
}
SMALL_FILMS = ["8x8", "24x16", "72x40", "200x120"]
# In those films the light stands at the eye, so a shadow ray runs back along its primary and next to none is occluded (only the film with the camera moved sideways has
# occluded rays): `NAME/side` is the same film with the light moved to the side of the soup, where a large part of the shadow rays is occluded -- deposits AND retractions
SIDE_LIGHT = (2.0, 1.2, 2.0)
SIDE_FILMS = [n + "/side" for n in SMALL_FILMS + ["400x300", "800x600"]]
_cache = {}


def _soup(w, h):
    return scenes.soup_scene(N_TRIS, w, h, half_extent=HALF)


def _with_material(sc, mat):
    return replace(sc, meshes=[replace(m, material=mat) for m in sc.meshes])


# Frames the early deposit must keep its hands off (each breaks ONE of the host's conditions), and `black`, which meets them all while EVERY shadow ray fails
# deposit_shadow's predicate: a LAMBERT colour of 0 shades to c = 0, the ray is emitted, traced and counted, and must never touch its pixel.
BUILDERS = {
    "two_lights": lambda: replace(_soup(72, 40), lights=np.concatenate([point_light((0.5, 0.5, 3.0)), point_light((1.5, 0.8, 2.5), (0.5, 0.25, 0.125))])),
    "samples_2x2": lambda: (lambda sc: replace(sc, camera=replace(sc.camera, samples=2)))(_soup(40, 24)),
    "depth_2": lambda: (lambda sc: replace(sc, camera=replace(sc.camera, depth=2)))(_soup(72, 40)),
    # (alpha = 1, Material()'s default: powf(x, 1) = x on the device and in libm alike; for other exponents the two differ in the last bit -- tests/test_gpu_native.py gives PHONG 1e-5)
    "phong": lambda: _with_material(_soup(72, 40), default_material(mtype=PHONG)),
    "two_instances": lambda: scenes.bunny_grid_scene(2, 1, width=96, height=64),
    "black": lambda: _with_material(_soup(72, 40), default_material(kd=(0.0, 0.0, 0.0))),
}


def _film(name):
    w, h, eye_x = FILMS[name]
    sc = _soup(w, h)
    if eye_x is not None:
        sc = replace(sc, camera=replace(sc.camera, eye=(eye_x, 0.5, 3.0), focus=(eye_x, 0.5, 0.5)))
    return sc


def case(name):
    """(scene, oracle frame, oracle stats) of a film, of a film lit from the side (NAME/side) or of a scene of BUILDERS."""
    if name not in _cache:
        sc = _film(name) if name in FILMS else replace(_film(name[:-5]), lights=point_light(SIDE_LIGHT)) if name.endswith("/side") else BUILDERS[name]()
        ref, st = oracle_render(sc, NORMALS_FLAT, nthreads=8)
        ref.setflags(write=False)
        _cache[name] = (sc, ref, st)
    return _cache[name]
