"""Volume domains across ranks, host side (no GPU): scheduler.VolumeDomainTracer -- DomainTracer's BSP and overlapped loops and its
composite -- over the numpy backend of tests/volume_domain_backend.py, ranks as threads on tests/fake_dist.FakeWorld.  The composited
image must equal volume_checker.frame bit for bit, the rays sent must be the brick-to-brick hops between bricks of different owners
(counted from the checker's own shuffle), and the loops must end.  Also: the header declares the new entry points at ABI revision 6."""
import functools
import os
import re

import numpy as np
import pytest

from gravit_amd import capi, scenes
from tests import volume_checker as vc
from tests import volume_domain_backend as vdb
from tests.conftest import ROOT

NEW = ["gvt_hip_volume_march_queue", "gvt_hip_volume_camera_filter", "gvt_hip_queues_export_wire", "gvt_hip_queues_append_wire"]


def test_header_declares_the_entry_points_and_the_abi_revision_stays():
    hdr = open(os.path.join(ROOT, "include", "gvt_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS
    assert int(re.search(r"#define GVT_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 6 and capi.ABI_VERSION == 6
    assert int(re.search(r"#define\s+GVT_HIP_MARCH_MAY_CLIP\s+(\d+)", hdr).group(1)) == capi.MARCH_MAY_CLIP


@functools.lru_cache(maxsize=None)
def reference(split, tf_kind, eye):
    """(bricks, camera, tf, the checker's frame, moves[a][b], marched[a]) of a case, computed once."""
    parts = scenes.split_volume(vdb.case_volume(), *vdb.SPLITS[split])
    tf, cam = vdb.case_tf(tf_kind), vdb.case_camera(eye)
    minv = scenes.instance_matrices(vdb.IDENT)[0]
    bricks = [vc.Brick(b, tf, vdb.RATE) for b in parts]
    lo, hi = [b.lo for b in parts], [b.hi for b in parts]
    want, _ = vc.frame(bricks, lo, hi, minv, cam)
    fb, moves, marched = vdb.hops(bricks, lo, hi, minv, cam)
    assert np.array_equal(fb.view(np.uint32), want.view(np.uint32))  # (the counting loop is the checker's frame)
    assert (want[..., 3] != 0).mean() > 0.25
    return parts, cam, tf, want, moves, marched


def sent_between_owners(moves, owner):
    return int(sum(moves[a, b] for a in range(len(owner)) for b in range(len(owner)) if owner[a] != owner[b]))


@pytest.mark.parametrize("overlap", [False, True], ids=["bsp", "overlapped"])
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("split,owner_kind,tf_kind,eye", [("2x2x2", "round_robin", "thin", "outside"), ("3x1x2", "checker", "dense", "inside"),
                                                         ("2x2x2", "last", "dense", "outside")])
def test_domain_loops_give_the_checkers_frame_and_its_hops(split, owner_kind, tf_kind, eye, world, overlap):
    parts, cam, tf, want, moves, marched = reference(split, tf_kind, eye)
    owner = vdb.case_owner(owner_kind, parts, world)
    res = vdb.numpy_run(parts, owner, world, cam, tf, vdb.RATE, overlap)
    assert sorted(res) == list(range(world))  # every rank ended
    img = res[0][0][0]
    assert np.array_equal(img.view(np.uint32), want.view(np.uint32))
    assert all(res[r][0][0] is None for r in range(1, world))
    sent = sum(res[r][0][1] for r in range(world))
    assert sent == sent_between_owners(moves, owner)
    if len(set(owner)) > 1:
        assert sent > 0
    for r in range(world):  # a rank that owns a brick the camera's rays reach marches
        if any(marched[i] for i in range(len(owner)) if owner[i] == r):
            assert res[r][0][3] >= 1
    if world == 1:
        assert res[0][0][2] == (0 if overlap else 1)  # one BSP round; the overlapped loop of one rank exchanges nothing


def test_checker_owner_map_separates_face_neighbours():
    for split in vdb.SPLITS:
        parts = scenes.split_volume(vdb.case_volume(), *vdb.SPLITS[split])
        for world in (2, 3, 8):
            owner = vdb.case_owner("checker", parts, world)
            for i, a in enumerate(parts):
                for j, b in enumerate(parts):
                    d = np.abs(a.offset - b.offset)
                    if (d > 0).sum() == 1 and d.max() == (a.counts - 1)[np.argmax(d)]:  # a shared face
                        assert owner[i] != owner[j], (split, world, i, j)
