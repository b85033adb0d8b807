"""Inputs the volume tests share, host and GPU alike (no device call at import): the colour / opacity tables read from
tests/golden/colormaps, the small noise grid with non-uniform spacing and the two instance matrices of tests/test_gpu_volume.py, and the
typed-voxel helpers of tests/test_gpu_volume_types.py."""
import os

import numpy as np

from gravit_amd import capi, scenes
from gravit_amd.adapter import TransferFunction
from tests.conftest import GOLDEN

F = np.float32
CMAPS = os.path.join(GOLDEN, "colormaps")
IDENT = scenes.mat_translate_scale((0, 0, 0), (1, 1, 1))
MOVED = scenes.mat_translate_scale((0.3, -0.2, 0.5), (1.5, 1.5, 1.5))


def read(name, width):
    return TransferFunction.read_map(os.path.join(CMAPS, name), width)


def tf(kind):
    cool = read("CoolWarm.cmap", 4)
    if kind == "cool":
        return TransferFunction(cool, read("CoolWarm.omap", 2), (0.0, 1.0))
    if kind == "spikes":  # sparse: opacity only around 0.9
        return TransferFunction(read("Grayramp.cmap", 4), read("fivespikes.omap", 2), (0.0, 1.0))
    if kind == "ramp":
        return TransferFunction(cool, read("ramp.omap", 2), (0.1, 0.8))
    if kind == "opaque":
        return TransferFunction(cool, np.array([[0, 1], [1, 1]], F), (0.0, 1.0))
    raise KeyError(kind)


def grid(n=24):
    vol = scenes.noise_volume(n, seed=3)
    vol.origin = np.array([-0.25, 0.1, -0.4], F)
    vol.spacing = np.array([1.0 / (n - 1), 1.1 / (n - 1), 0.9 / (n - 1)], F)
    return vol


# per type: numpy dtype, the library's constant, the image of noise_volume's [0, 1] (the transfer functions' value range), the quantiser,
# and a value just across the sign bit
TYPES = {
    "u8": (np.uint8, capi.VOXEL_U8, (0.0, 255.0), lambda d: np.rint(d * 255.0), 128),
    "i16": (np.int16, capi.VOXEL_I16, (-30000.0, 30000.0), lambda d: np.rint((d - 0.5) * 60000.0), -1),
    "u16": (np.uint16, capi.VOXEL_U16, (0.0, 65535.0), lambda d: np.rint(d * 65535.0), 32768),
}
ALL = sorted(TYPES)


def quantised(vol, ty):
    """The [0, 1] grid in the type's units, geometry kept."""
    q = np.ascontiguousarray(TYPES[ty][3](vol.data.astype(np.float64)).astype(TYPES[ty][0]))
    return scenes.VolumeData(q, vol.origin, vol.spacing)


def as_float(vol):
    return scenes.VolumeData(vol.data.astype(F), vol.origin, vol.spacing)


def scaled(kind, ty, value_range=None):
    """tests.test_gpu_volume.tf's tables with the value range in the type's units (or the one given)."""
    t = tf(kind)
    lo, hi = TYPES[ty][2]
    vr = value_range or tuple(lo + r * (hi - lo) for r in t.value_range)
    return TransferFunction(t.cmap, t.omap, vr)
