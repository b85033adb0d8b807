"""Time-varying volumes, host side (no GPU): gvt_hip_volume_update_samples is declared, bound and exported without an ABI bump, the numpy
restatement of the macro cells' ranges (tests/volume_range_checker.py) equals a brute-force walk over the cells, and the Python layer refuses
a wrong shape, dtype or bricking before it reaches the device."""
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import HipVolumeAdapter, TransferFunction
from gravit_amd.scheduler import VolumeTracer
from tests import volume_range_checker as rc
from tests.conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAME = "gvt_hip_volume_update_samples"


def header():
    return open(os.path.join(ROOT, "include", "gvt_hip.h")).read()


def test_header_declares_the_entry_point():
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, header())
    assert m, NAME
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert args == ["gvt_hip_volume *", "const float *samples", "size_t n_samples", "uint32_t flags", "float *ms_out"]
    assert re.search(r"#define\s+GVT_HIP_UPDATE_DEVICE\s+1u", header())


def test_binding_lists_it_and_the_abi_is_still_6():
    assert NAME in capi.SYMBOLS
    assert capi.ABI_VERSION == 6 and re.search(r"#define\s+GVT_HIP_ABI_VERSION\s+6\b", header())


def test_library_exports_it():
    so = capi.LIB_PATH
    if not os.path.exists(so):
        pytest.fail("%s is missing: build() first" % so)
    exported = set(re.findall(r" T (gvt_hip_\w+)", subprocess.run(["nm", "-D", so], check=True, stdout=subprocess.PIPE, text=True).stdout))
    assert NAME in exported
    assert capi.load().gvt_hip_abi_version() == 6


def test_python_layer_has_the_calls():
    assert callable(getattr(HipVolumeAdapter, "update_samples", None))
    assert callable(getattr(VolumeTracer, "update", None))


def special(shape, seed):
    """Noise with a NaN, a +Inf, a -Inf and a huge pair on random vertices (x y z counts)."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    d = rng.random((nz, ny, nx), dtype=np.float32)
    for v in (np.nan, np.inf, -np.inf, 3e38, -3e38):
        d[rng.integers(nz), rng.integers(ny), rng.integers(nx)] = v
    return d


@pytest.mark.parametrize("shape", [(2, 2, 2), (10, 9, 18), (17, 17, 17), (9, 2, 3), (3, 26, 8)])
def test_range_restatement_equals_a_walk_over_the_cells(shape):
    for seed in range(3):
        d = special(shape, seed)
        a, b = rc.ranges(d), rc.ranges_by_cells(d)
        assert a[0].shape == tuple(rc.blocks(d.shape))
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    nan = np.full((3, 9, 10), np.nan, F)  # nothing but NaN: the bounds stay +Inf / -Inf
    nan[0, 0, 9] = 2.0                    # ... except in the second block along x
    mn, mx, wild = rc.ranges(nan)
    assert mn[0, 0, 0] == np.inf and mx[0, 0, 0] == -np.inf and wild.all()
    assert mn[0, 0, 1] == mx[0, 0, 1] == 2.0
    assert rc.value_range(nan) == (F(2.0), F(2.0))
    shared = np.zeros((2, 2, 17), F)      # a vertex on a block boundary counts for both blocks
    shared[1, 1, 8] = 5.0
    assert rc.ranges(shared)[1].reshape(-1).tolist() == [5.0, 5.0]
    shared[1, 1, 8] = np.inf
    assert rc.ranges(shared)[2].all() and (rc.ranges(shared)[1] == np.inf).all()


def test_empty_rule_restatement():
    rd = TransferFunction.read_map
    cm = os.path.join(GOLDEN, "colormaps")
    spikes = TransferFunction(rd(os.path.join(cm, "Grayramp.cmap"), 4), rd(os.path.join(cm, "fivespikes.omap"), 2), (0.0, 1.0))  # opaque around 0.9 only
    d = np.zeros((2, 2, 33), F)           # four blocks along x
    assert rc.n_blocks_empty(d, spikes) == 4
    d[0, 0, 16] = 0.9                     # shared by blocks 1 and 2
    assert rc.empty_blocks(d, spikes).reshape(-1).tolist() == [True, False, False, True]
    d[0, 0, 16] = 0.8                     # below the spike, beyond the margin
    assert rc.n_blocks_empty(d, spikes) == 4
    d[0, 0, 3] = np.nan                   # a NaN sample looks up entry 0, which is transparent here
    assert rc.n_blocks_empty(d, spikes) == 4
    d[0, 0, 3] = np.inf                   # max = +Inf: entry 255 and everything below
    assert rc.empty_blocks(d, spikes).reshape(-1).tolist() == [False, True, True, True]
    d[0, 0, 3], d[0, 0, 4] = 3e38, -3e38  # finite, but a lerp between them overflows: the whole table
    assert rc.empty_blocks(d, spikes).reshape(-1).tolist() == [False, True, True, True]


def test_update_samples_refuses_shape_and_dtype_before_the_library():
    fake = SimpleNamespace(counts=np.array([4, 3, 2], np.int32))  # no lib, no handle: reaching the library would raise AttributeError
    with pytest.raises(ValueError, match="shape"):
        HipVolumeAdapter.update_samples(fake, np.zeros((4, 3, 2), F))
    with pytest.raises(ValueError, match="shape"):
        HipVolumeAdapter.update_samples(fake, np.zeros(24, F))
    with pytest.raises(ValueError, match="float32"):
        HipVolumeAdapter.update_samples(fake, np.zeros((2, 3, 4), np.float64))


def test_update_refuses_another_bricking():
    vol = scenes.noise_volume(24, seed=1)
    pushed = []
    ads = [SimpleNamespace(counts=b.counts, offset=b.offset, update_samples=pushed.append) for b in scenes.split_volume(vol, 2, 2, 1)]
    tr = SimpleNamespace(adapters=ads, _same_bricking=VolumeTracer._same_bricking)
    nxt = scenes.noise_volume(24, seed=2)
    for other in (scenes.split_volume(nxt, 1, 2, 2), scenes.split_volume(nxt, 2, 1, 1), nxt, scenes.split_volume(scenes.noise_volume(25), 2, 2, 1)):
        with pytest.raises(ValueError, match="brick"):
            VolumeTracer.update(tr, other)
    assert not pushed                     # nothing reached a brick
    moved = scenes.split_volume(nxt, 2, 2, 1)
    moved[3].offset = moved[3].offset + 1  # the same counts somewhere else
    with pytest.raises(ValueError, match="offset"):
        VolumeTracer.update(tr, moved)
    same = scenes.split_volume(nxt, 2, 2, 1)
    assert VolumeTracer.update(tr, same) is tr
    assert len(pushed) == 4 and all(p is b.data for p, b in zip(pushed, same))
    one = SimpleNamespace(adapters=[SimpleNamespace(counts=vol.counts, offset=np.zeros(3, np.int32), update_samples=pushed.append)],
                          _same_bricking=VolumeTracer._same_bricking)
    assert VolumeTracer.update(one, nxt) is one and pushed[-1] is nxt.data  # one VolumeData: the whole grid as one brick
