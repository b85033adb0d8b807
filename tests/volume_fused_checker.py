"""numpy restatement of the fused frame (include/gvt_hip.h, "fused frame"; gravit_amd/csrc/volume_fused.inc): every camera ray is followed
to its end -- first brick, visit, next brick, ... deposit -- instead of being passed through per-brick queues.  The visits and the
next-brick rule are tests/volume_checker.py's march and next_brick (with a depth plane: tests/volume_clip_checker.py's), so what this file
adds is only the order of work: rays grouped by the brick they are in now, one ray-set at a time, no queues, no rounds.
tests/test_volume_fused_host.py shows that it gives volume_checker.frame's bits and the same number of (ray, brick) visits."""
import numpy as np

from oracle import orc
from tests import volume_checker as vc
from tests import volume_clip_checker as cc

F = np.float32


def frame(bricks, lo, hi, minv, cam, plane=None):
    """gvt_hip_volume_frame_fused: the (H, W, 4) un-clamped framebuffer and the counters {brick_visits, rays_deposited}.  plane: (H, W)
    floats (the clipped frame), or None."""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    fb = np.zeros((cam.width * cam.height, 4), F)
    rays = vc.camera_rays(cam)
    rays["color"] = 0  # a camera ray starts with no colour, no opacity and no flags
    rays["w"] = 0
    rays["depth"] = 0
    if plane is None:
        march, next_brick = vc.march, vc.next_brick
    else:
        march, next_brick = cc.march, cc.next_brick
        ids = rays["id"].astype(np.int64)
        inside = (ids >= 0) & (ids < cam.width * cam.height)
        t = np.where(inside, np.ascontiguousarray(plane, F).reshape(-1)[np.where(inside, ids, 0)], F(np.inf)).astype(F)
        rays["t_max"] = np.where(inside, t, rays["t_max"])
        with np.errstate(all="ignore"):
            rays["depth"] = np.where(t < F(np.inf), cc.CLIP, 0)
    brick = next_brick(lo, hi, order, rays, -1)
    rays, brick = rays[brick >= 0], brick[brick >= 0]  # no first brick: dropped, nothing deposited
    visits = deposits = 0
    while len(rays):
        b = int(brick[0])  # one ray-set: the rays that are in brick b now
        here = brick == b
        visits += int(here.sum())
        out = march(bricks[b], rays[here], minv)
        opaque = (out["depth"] & vc.OPAQUE) != 0
        out["depth"] &= ~(vc.OPAQUE | vc.BOUNDARY)  # (the flags are the loop's way of passing the decision on; here it is taken at once)
        nxt = np.full(len(out), -1, np.int64)
        if (~opaque).any():
            nxt[~opaque] = next_brick(lo, hi, order, out[~opaque], b)
        done = nxt < 0  # OPAQUE, or EXTERNAL
        dep = out[done]
        ids = dep["id"].astype(np.int64)
        ok = (ids >= 0) & (ids < len(fb))
        np.add.at(fb, (ids[ok], slice(0, 3)), dep["color"][ok])
        np.add.at(fb, (ids[ok], 3), dep["w"][ok])
        deposits += int(done.sum())
        rays = np.concatenate([rays[~here], out[~done]])
        brick = np.concatenate([brick[~here], nxt[~done]])
    return fb.reshape(cam.height, cam.width, 4), {"brick_visits": visits, "rays_deposited": deposits}
