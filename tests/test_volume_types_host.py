"""Typed voxels, host side (no GPU): scenes.read_bov(native=True), split_volume on integer grids, the voxel-type constants."""
import os
import re

import numpy as np

from gravit_amd import capi, scenes
from tests.conftest import ROOT

F = np.float32


def write_bov(tmp_path, name, data, fmt, endian=None):
    """data[z, y, x] as a .bov header and its raw file; data's own byte order goes to disk."""
    nz, ny, nx = data.shape
    data.tofile(str(tmp_path / (name + ".raw")))
    lines = ["DATA_FILE: %s.raw" % name, "DATA_SIZE: %d %d %d" % (nx, ny, nz), "DATA_FORMAT: %s" % fmt, "VARIABLE: v",
             "BRICK_ORIGIN: 1 2 3", "BRICK_SIZE: %d %d %d" % (2 * (nx - 1), ny - 1, nz - 1)]
    if endian:
        lines.append("DATA_ENDIAN: %s" % endian)
    path = tmp_path / (name + ".bov")
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_read_bov_native_keeps_the_integer_types(tmp_path):
    rng = np.random.default_rng(4)
    shape = (3, 4, 5)
    u8 = rng.integers(0, 256, shape).astype(np.uint8)
    u8[0, 0, :2] = (0, 255)
    i16 = rng.integers(-32768, 32768, shape).astype(np.int16)
    i16[0, 0, :3] = (-32768, 32767, -1)
    f32 = rng.random(shape).astype(F)
    cases = [(write_bov(tmp_path, "u", u8, "UCHAR"), u8, np.uint8),
             (write_bov(tmp_path, "b", u8, "BYTE"), u8, np.uint8),
             (write_bov(tmp_path, "s", i16.astype(">i2"), "SHORT", "BIG"), i16, np.int16),
             (write_bov(tmp_path, "l", i16.astype("<i2"), "SHORT", "LITTLE"), i16, np.int16),
             (write_bov(tmp_path, "f", f32, "FLOAT"), f32, np.float32),
             (write_bov(tmp_path, "i", i16.astype("<i4"), "INT"), i16.astype(F), np.float32)]  # INT is not exact in float32: converted
    for path, want, native_t in cases:
        hdr, vol = scenes.read_bov(path, native=True)
        assert vol.data.dtype == np.dtype(native_t) and vol.data.dtype.isnative and vol.data.flags["C_CONTIGUOUS"], path
        assert vol.data.shape == shape and (vol.data == want).all(), path
        hdr0, old = scenes.read_bov(path)  # the default: float32 with the same values as before
        assert old.data.dtype == np.float32 and (old.data == want.astype(F)).all(), path
        assert hdr == hdr0 and (vol.origin == old.origin).all() and (vol.spacing == old.spacing).all()
        assert vol.origin.tolist() == [1.0, 2.0, 3.0] and vol.spacing.tolist() == [2.0, 1.0, 1.0]


def test_split_volume_keeps_the_dtype_and_the_shared_layers():
    rng = np.random.default_rng(2)
    for np_t in (np.uint8, np.int16, np.uint16):
        lim = np.iinfo(np_t)
        data = rng.integers(lim.min, lim.max + 1, (9, 11, 14)).astype(np_t)
        vol = scenes.VolumeData(data, np.array([0.5, 0, -1], F), np.array([0.1, 0.2, 0.3], F))
        parts = scenes.split_volume(vol, 3, 2, 2)
        want = scenes.split_volume(scenes.VolumeData(data.astype(F), vol.origin, vol.spacing), 3, 2, 2)
        assert len(parts) == 12
        cells = 0
        for p, w in zip(parts, want):
            assert p.data.dtype == np.dtype(np_t) and p.data.flags["C_CONTIGUOUS"]
            assert (p.data.astype(F) == w.data).all() and (p.offset == w.offset).all() and (p.lo == w.lo).all() and (p.hi == w.hi).all()
            o, c = p.offset, p.counts
            assert (p.data == data[o[2]:o[2] + c[2], o[1]:o[1] + c[1], o[0]:o[0] + c[0]]).all()
            cells += int(np.prod(c - 1))
        assert cells == 8 * 10 * 13  # every cell owned once: neighbours share their boundary layer of vertices
        a, b = parts[0], parts[1]  # neighbours along x
        assert a.offset[0] + a.counts[0] - 1 == b.offset[0] and (a.data[:, :, -1] == b.data[:, :, 0]).all()


def test_voxel_type_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "gvt_hip.h")).read()
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define GVT_HIP_VOXEL_(\w+)\s+(\d+)\s*$", hdr, re.M)}
    assert found == {"F32": 0, "U8": 1, "I16": 2, "U16": 3}
    assert (capi.VOXEL_F32, capi.VOXEL_U8, capi.VOXEL_I16, capi.VOXEL_U16) == (found["F32"], found["U8"], found["I16"], found["U16"])
    assert capi.VOXEL_TYPES == {"float32": capi.VOXEL_F32, "uint8": capi.VOXEL_U8, "int16": capi.VOXEL_I16, "uint16": capi.VOXEL_U16}
    for name in ("gvt_hip_volume_create_typed", "gvt_hip_volume_update_samples_typed", "gvt_hip_volume_get_voxel_type"):
        assert name in capi.SYMBOLS and re.search(r"\b%s\(" % name, hdr)
    assert re.search(r"#define GVT_HIP_ABI_VERSION 6\b", hdr) and capi.ABI_VERSION == 6
