"""Volume domains, host side (no GPU): GraviT's colour-map formats and their 256-entry resampling, the BOV reader, the bricking of a grid,
and the numpy checker's own invariants -- a bricked frame equals the whole frame bit for bit, and a sample of zero opacity adds exactly +0
(what makes macro-cell skipping exact)."""
import os
import re

import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import TransferFunction
from tests import volume_checker as vc
from tests.conftest import GOLDEN, ROOT

F = np.float32
CMAPS = os.path.join(GOLDEN, "colormaps")
NEW = ["gvt_hip_volume_create", "gvt_hip_volume_destroy", "gvt_hip_volume_get_info", "gvt_hip_volume_set_transfer", "gvt_hip_volume_trace",
       "gvt_hip_shuffle_volume", "gvt_hip_volume_frame"]


def test_header_declares_and_binding_lists_the_volume_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gvt_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS
    for flag, v in (("GVT_HIP_RAY_OPAQUE", 0x2), ("GVT_HIP_RAY_BOUNDARY", 0x4), ("GVT_HIP_RAY_EXTERNAL_BOUNDARY", 0x10)):
        assert int(re.search(r"#define\s+%s\s+(0x[0-9a-f]+)" % flag, hdr).group(1), 16) == v
    assert capi.RAY_OPAQUE == 0x2 and capi.RAY_BOUNDARY == 0x4 and capi.RAY_EXTERNAL_BOUNDARY == 0x10
    import ctypes as C

    assert C.sizeof(capi.VolumeInfo) == 88


def test_map_parser_reads_counts_then_rows(tmp_path):
    p = tmp_path / "a.omap"
    p.write_text("3\n0.0 0.0 \n0.5 1.0\n1.0 0.25\n")
    m = TransferFunction.read_map(str(p), 2)
    assert m.dtype == F and m.shape == (3, 2)
    assert m.tolist() == [[0.0, 0.0], [0.5, 1.0], [1.0, 0.25]]
    q = tmp_path / "short.cmap"
    q.write_text("2\n0 1 1 1\n")
    with pytest.raises(ValueError):
        TransferFunction.read_map(str(q), 4)


@pytest.mark.parametrize("name,width,rows", [("Grayramp.cmap", 4, 2), ("Grayramp.omap", 2, 4), ("CoolWarm.cmap", 4, 3), ("CoolWarm.omap", 2, 11),
                                             ("fivespikes.omap", 2, 20), ("ramp.omap", 2, 2)])
def test_reference_colormaps_parse(name, width, rows):
    m = TransferFunction.read_map(os.path.join(CMAPS, name), width)
    assert m.shape == (rows, width)
    assert (np.diff(m[:, 0]) >= 0).all()


def test_resampling_matches_hand_computed_entries():
    ramp = TransferFunction.read_map(os.path.join(CMAPS, "ramp.omap"), 2)  # (0, 0) .. (1, 0.5)
    t = vc.resample(ramp, 2)[:, 0]
    assert t[0] == 0 and t[255] == F(0.5)
    x51 = F(51 / 255.0)  # x = 0.2 (rounded to float), d = x / 1, a = 0 + d * 0.5
    assert t[51] == F(x51 * F(0.5))
    gray = TransferFunction.read_map(os.path.join(CMAPS, "Grayramp.omap"), 2)  # 1 up to x = 0.5, 0 from x = 0.51
    g = vc.resample(gray, 2)[:, 0]
    assert (g[:128] == 1).all() and (g[131:] == 0).all()  # x_127 = 0.498, x_131 = 0.514
    cool = TransferFunction.read_map(os.path.join(CMAPS, "CoolWarm.cmap"), 4)
    c = vc.resample(cool, 4)
    # the last entry interpolates the last segment at d = 1: a + 1 * (b - a), which need not be b in float
    assert c[0].tolist() == cool[0, 1:].tolist() and c[255].tolist() == (cool[1, 1:] + (cool[2, 1:] - cool[1, 1:])).tolist()
    assert c[255, 2] != cool[2, 3]
    # opacity correction: a' = 1 - (1 - a)^(1 / rate) in double, rounded once
    tab = vc.table(cool, ramp, 2.0)
    assert tab[255, 3] == F(1.0 - (1.0 - 0.5) ** 0.5) and tab[0, 3] == 0
    assert (vc.table(cool, ramp, 1.0)[:, 3] == t).all()


def test_read_bov_header_fixture(tmp_path):
    hdr = open(os.path.join(GOLDEN, "sphere.bov")).read()
    assert "DATA_SIZE: 100 100 100" in hdr and "DATA_FORMAT: FLOAT" in hdr
    # the same header over a tiny data file of each supported type
    for fmt, dt in (("FLOAT", "<f4"), ("INT", "<i4"), ("UCHAR", "u1")):
        small = re.sub(r"DATA_SIZE:.*", "DATA_SIZE: 3 4 5", hdr)
        small = re.sub(r"DATA_FORMAT:.*", "DATA_FORMAT: %s" % fmt, small)
        (tmp_path / "sphere.bov").write_text(small)
        vals = np.arange(60).astype(dt)
        vals.tofile(str(tmp_path / "sphere"))
        h, vol = scenes.read_bov(str(tmp_path / "sphere.bov"))
        assert h["VARIABLE"] == "density"
        assert vol.data.dtype == F and vol.data.shape == (5, 4, 3)
        assert (vol.data.reshape(-1) == np.arange(60, dtype=F)).all()
        assert vol.counts.tolist() == [3, 4, 5]


@pytest.mark.parametrize("split", [(1, 1, 1), (2, 2, 2), (4, 2, 1), (1, 1, 8), (3, 2, 5)])
def test_split_volume_covers_every_cell_once(split):
    vol = scenes.VolumeData(np.random.default_rng(1).random((17, 13, 11), dtype=F), np.array([0.5, -1, 2], F), np.array([0.25, 0.5, 0.125], F))
    bricks = scenes.split_volume(vol, *split)
    assert len(bricks) == split[0] * split[1] * split[2]
    owned = np.zeros((16, 12, 10), np.int32)
    for b in bricks:
        o, n = b.offset, b.counts
        owned[o[2]:o[2] + n[2] - 1, o[1]:o[1] + n[1] - 1, o[0]:o[0] + n[0] - 1] += 1
        assert (b.data == vol.data[o[2]:o[2] + n[2], o[1]:o[1] + n[1], o[0]:o[0] + n[0]]).all()  # shares one vertex layer
        assert (b.lo == (vol.origin + o.astype(F) * vol.spacing).astype(F)).all()
    assert (owned == 1).all()


def test_zero_opacity_sample_adds_exactly_zero():
    rng = np.random.default_rng(5)
    C = rng.random((100000, 3), dtype=F)
    A = (rng.random(100000, dtype=F) * F(0.99)).astype(F)
    c = rng.random((100000, 3), dtype=F)
    f = ((F(1) - A) * F(0)).astype(F)
    assert ((C + f[:, None] * c).view(np.uint32) == C.view(np.uint32)).all()
    assert ((A + f).view(np.uint32) == A.view(np.uint32)).all()


def _tf(kind):
    cool = TransferFunction.read_map(os.path.join(CMAPS, "CoolWarm.cmap"), 4)
    if kind == "spikes":
        return TransferFunction(cool, TransferFunction.read_map(os.path.join(CMAPS, "fivespikes.omap"), 2), (0.0, 1.0))
    return TransferFunction(cool, TransferFunction.read_map(os.path.join(CMAPS, "CoolWarm.omap"), 2), (0.0, 1.0))


def small_camera(w=40, h=32):
    return scenes.Camera((2.3, 1.7, 3.1), (0.48, 0.51, 0.47), (0.0, 1.0, 0.0), float(F(40.0 * np.pi / 180.0)), w, h)


@pytest.mark.parametrize("split", [(2, 2, 2), (4, 2, 1), (1, 1, 8)])
def test_checker_bricked_frame_equals_whole_frame(split):
    vol = scenes.sphere_volume(17)
    vol.spacing = np.full(3, F(1.0 / 16), F)
    tf = _tf("cool")
    cam = small_camera()
    minv = scenes.instance_matrices(scenes.mat_translate_scale((0, 0, 0), (1, 1, 1)))[0]
    whole = vc.Brick(vol, tf, 1.5)
    fb1, calls1 = vc.frame([whole], whole.lo[None], whole.hi[None], minv, cam)
    assert calls1 == 1 and (fb1[..., 3] > 0).sum() > 100
    parts = scenes.split_volume(vol, *split)
    bricks = [vc.Brick(b, tf, 1.5) for b in parts]
    fbn, calls = vc.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], minv, cam)
    assert calls >= len(parts) - 1
    assert (fbn.view(np.uint32) == fb1.view(np.uint32)).all()
