"""The cases of the fused-frame tests (tests/test_gpu_volume_fused.py, tests/test_volume_fused_host.py): the smallest shapes at which the
kernel can still go wrong -- a 25^3 noise grid with non-uniform spacing, a 64 x 48 film at one sample per pixel, sampling rate 1.7, cut
into 1, 8, 6 and 64 bricks (the last: bricks of 6 cells, every macro cell partial, more bricks than most rays visit) -- and the checker's
frames of them, computed once per case and shared."""
import functools

import numpy as np

from gravit_amd import scenes
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests.volume_common import IDENT, MOVED, grid, tf

F = np.float32
RATE = 1.7
N = 25
FILM = (64, 48)
SPLITS = [(1, 1, 1), (2, 2, 2), (3, 1, 2), (4, 4, 4)]
TABLES = ["cool", "spikes", "opaque"]
FOV = float(F(35.0 * np.pi / 180.0))


def volume(seed=3):
    vol = grid(N)
    if seed != 3:  # another time step on the same geometry
        vol.data = scenes.noise_volume(N, seed=seed).data
    return vol


def bricks_of(vol, split):
    return scenes.split_volume(vol, *split)


def matrix(moved):
    return MOVED if moved else IDENT


def to_world(m, p):
    M = np.asarray(m, np.float64).reshape(4, 4).T
    return tuple(float(v) for v in (np.asarray(p, np.float64) @ M[:3, :3].T + M[:3, 3]))


def camera(where, moved=False):
    """outside: an eye beside the volume looking at its middle; inside: an eye inside a brick (in every bricking used here) looking
    through the volume; away: the outside eye looking away from it.  The points are given in the volume's own space and placed by m."""
    m = matrix(moved)
    vol = grid(N)
    lo = vol.origin.astype(np.float64)
    ext = (vol.counts - 1) * vol.spacing.astype(np.float64)
    mid = lo + 0.5 * ext
    out_eye = lo + ext * np.array([2.3, 1.6, 3.1])
    if where == "outside":
        eye, focus = out_eye, mid + ext * np.array([-0.02, 0.01, -0.03])
    elif where == "inside":
        eye, focus = lo + ext * np.array([0.37, 0.55, 0.61]), lo + ext * np.array([0.42, 0.42, 0.125])
    elif where == "away":
        eye, focus = out_eye, out_eye + (out_eye - mid)
    else:
        raise KeyError(where)
    return scenes.Camera(to_world(m, eye), to_world(m, focus), (0.0, 1.0, 0.0), FOV, FILM[0], FILM[1])


def world_boxes(parts, m):
    from gravit_amd.scheduler import _brick_boxes

    return _brick_boxes(parts, m)


@functools.lru_cache(maxsize=None)
def reference(split, table, moved, where, seed=3):
    """volume_checker.frame of the case: (framebuffer, [(brick, rays) per round], rays with a first brick).  Computed once; treat as
    read-only."""
    parts = bricks_of(volume(seed), split)
    m = matrix(moved)
    minv = scenes.instance_matrices(m)[0]
    lo, hi = world_boxes(parts, m)
    cam = camera(where, moved)
    bricks = [vc.Brick(b, tf(table), RATE) for b in parts]
    rounds = []
    fb, calls = vc.frame(bricks, lo, hi, minv, cam, rounds=rounds)
    from oracle import orc

    first = vc.next_brick(lo, hi, orc.toplevel_order(lo, hi), vc.camera_rays(cam), -1)
    fb.setflags(write=False)
    return fb, tuple(rounds), int((first >= 0).sum())


def depth_plane(parts, moved, where="outside"):
    """A (H, W) depth plane that mixes, pixel by pixel: +Inf, depths in front of every brick, depths inside the volume, depths beyond it,
    and -- one pixel -- a depth a quarter of a lattice step behind the face where the ray leaves its first brick."""
    m = matrix(moved)
    cam = camera(where, moved)
    lo, hi = world_boxes(parts, m)
    rays = vc.camera_rays(cam)
    o, d = rays["origin"].astype(F), rays["direction"].astype(F)
    tn, tf_ = vc.slab(lo.min(axis=0), hi.max(axis=0), o, d)
    hit = (tn <= tf_) & (tf_ > 0)
    tn = np.where(hit, np.maximum(tn, F(0)), F(0.5))
    tf_ = np.where(hit, tf_, F(1.0))
    ids = rays["id"].astype(np.int64)
    u = np.random.default_rng(8).random(len(rays)).astype(F)
    kind = ids % 5
    t = np.full(len(rays), np.inf, F)
    t = np.where(kind == 1, F(0.5) * tn, t)
    t = np.where((kind == 2) | (kind == 4), tn + (tf_ - tn) * u, t)
    t = np.where(kind == 3, F(1.5) * tf_, t)
    # the pixel in the middle of the film: just behind the exit face of its first brick
    from oracle import orc

    mid = int(np.nonzero(ids == (FILM[1] // 2) * FILM[0] + FILM[0] // 2)[0][0])
    first = int(vc.next_brick(lo, hi, orc.toplevel_order(lo, hi), rays[mid:mid + 1], -1)[0])
    assert first >= 0
    dt = vc.Brick(parts[0], tf("cool"), RATE).dt
    t[mid] = vc.slab(lo[first], hi[first], o[mid:mid + 1], d[mid:mid + 1])[1][0] + F(0.25) * dt
    plane = np.full(FILM[0] * FILM[1], np.inf, F)
    plane[ids] = t
    return plane.reshape(FILM[1], FILM[0])


@functools.lru_cache(maxsize=None)
def clip_reference(split, table, moved):
    parts = bricks_of(volume(), split)
    m = matrix(moved)
    minv = scenes.instance_matrices(m)[0]
    lo, hi = world_boxes(parts, m)
    plane = depth_plane(parts, moved)
    fb, _ = cc.frame([vc.Brick(b, tf(table), RATE) for b in parts], lo, hi, minv, camera("outside", moved), plane)
    fb.setflags(write=False)
    return fb, plane
