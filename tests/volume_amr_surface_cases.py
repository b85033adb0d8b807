"""What the shaded AMR tests share (tests/test_volume_amr_surfaces_host.py, tests/test_gpu_volume_amr_surfaces.py): the surfaces and the
light set on tests/volume_amr_cases.py's scene, a ray set aimed at the level-2 subgrid S1, and a scene whose S0 holds a value level 0
never reaches."""
import numpy as np

from gravit_amd import scenes
from gravit_amd.layouts import RAY_DTYPE
from tests import volume_amr_cases as cases
from tests import volume_surface_checker as sc

F = np.float32
ISOVALUES = (0.5, 0.52)
LIGHTS = [((3.0, 4.0, 5.0), (1.0, 0.9, 0.8))]
KA, KD = 0.4, 0.6
PEAK, PEAK_ISO = 2.0, 1.5


def s0_plane(vol):
    """A slice plane (nx, ny, nz, d), object space, through the centre of S0's box and oblique to every axis."""
    org, sp = np.asarray(vol.origin, np.float64), np.asarray(vol.spacing, np.float64)
    mid = org + (np.array(cases.S0["lo"]) + 0.5 * np.array(cases.S0["cells"])) * sp
    nrm = np.array([0.3, 0.5, 1.0])
    return tuple(float(F(x)) for x in (*nrm, mid @ nrm))


def surfaces(vol, isovalues=ISOVALUES, plane=True, lights=True, ka=KA, kd=KD, opacity=0.7):
    """The checker's Surfaces; .args / .light_args are what HipVolumeAdapter.set_surfaces / set_lights take."""
    S = sc.Surfaces(isovalues, [s0_plane(vol)] if plane else [], opacity, LIGHTS if lights else [], ka, kd)
    S.args = dict(isovalues=list(isovalues), slices=[s0_plane(vol)] if plane else [], opacity=opacity)
    S.light_args = dict(lights=LIGHTS if lights else [], ka=ka, kd=kd)
    return S


def s1_box(vol):
    """The box of S1 (S0's ratio-4 child, level 2) in object space: lo and extent."""
    org, sp = np.asarray(vol.origin, F), np.asarray(vol.spacing, F)
    r0 = F(cases.S0["ratio"])
    lo = (org + (np.array(cases.S0["lo"], F) + np.array(cases.S1["lo"], F) / r0) * sp).astype(F)
    ext = (np.array(cases.S1["cells"], F) / r0 * sp).astype(F)
    return lo, ext


def s1_rays(vol, m, n=300, seed=11):
    """Rays aimed at S1's box, modelled on cases.plane_rays: origins around S0's box, targets inside S1; every third ray runs IN a vertex
    plane of S1 (d[a] == 0 in object space, the origin on a plane of S1's vertices: eighths of a level-0 cell)."""
    rng = np.random.default_rng(seed)
    org, sp = np.asarray(vol.origin, F), np.asarray(vol.spacing, F)
    lo, ext = s1_box(vol)
    o = (lo + ext * rng.random((n, 3)) + np.array([0.3, 0.4, 0.5]) * np.sign(rng.random((n, 3)) - 0.5)).astype(F)
    tgt = (lo + ext * rng.random((n, 3))).astype(F)
    d = (tgt - o).astype(F)
    third = np.arange(n) % 3 == 0
    a = (np.arange(n) // 3) % 3
    total = cases.S0["ratio"] * cases.S1["ratio"]
    eighth = rng.integers(0, cases.S1["cells"][0] * cases.S1["ratio"] + 1, n)  # (the smallest extent of S1 in its own vertices: 12)
    first = (np.array(cases.S0["lo"], F) + np.array(cases.S1["lo"], F) / F(cases.S0["ratio"]))[a]
    on_plane = (org[a] + (first + eighth.astype(F) / F(total)) * sp[a]).astype(F)
    idx = np.arange(n)[third]
    o[idx, a[third]] = on_plane[third]
    d[idx, a[third]] = 0
    M = np.asarray(m, F).reshape(4, 4).T
    r = np.zeros(n, RAY_DTYPE)
    r["origin"] = (o @ M[:3, :3].T + M[:3, 3]).astype(F)
    r["direction"] = (d @ M[:3, :3].T).astype(F)
    r["t_min"] = F(1e-6)
    r["t_max"] = np.finfo(F).max
    r["id"] = np.arange(n)
    return r


def peak_scene():
    """cases.scene() with a block of S0's vertices at PEAK, a value level 0 never reaches: S0's vertices x 7..11, y 5..9, z 9..15 (clear of
    S1's footprint, across the macro-cell planes x = 8 and z = 8).  Only the merged ranges know that PEAK_ISO is crossed there."""
    vol = cases.scene()
    s0 = vol.subgrids[0]
    data = s0.data.copy()
    data[9:16, 5:10, 7:12] = PEAK
    vol.subgrids[0] = scenes.Subgrid(s0.parent, s0.ratio, s0.lo, s0.cells, data)
    assert float(vol.data.max()) < PEAK_ISO
    return vol
