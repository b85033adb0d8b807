"""numpy restatement of the shaded fused frame (include/gvt_hip.h, "fused frame: surfaces and lit fog"; gravit_amd/csrc/
volume_fused_shaded.inc): tests/volume_fused_checker.py's per-ray formulation -- every camera ray followed from brick to brick until it
deposits, no queues, no rounds -- with two changes: the visit is tests/volume_shade_checker.py's march (surfaces, lit fog, the clip), and
the next brick is tests/volume_clip_checker.py's rule.  Between two visits only OPAQUE | BOUNDARY are cleared: the SIDES flag and the
side mask in the ray's t field stay, as does t_min -- the states the loop's ray passes through.  tests/test_volume_fused_shaded_host.py
shows that it gives volume_shade_checker.frame's bits and counts."""
import numpy as np

from oracle import orc
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_shade_checker as lc
from tests import volume_surface_checker as sc

F = np.float32


def frame(bricks, lo, hi, minv, cam, S=None, mode=lc.SHADE_GRADIENT, plane=None, keep_sides=True):
    """gvt_hip_volume_frame_fused_shaded with S and the mode on every brick: the (H, W, 4) un-clamped framebuffer and the counters
    {brick_visits, rays_deposited, crossings_rendered, samples_shaded}.  plane: (H, W) floats (the clipped frame), or None.
    keep_sides=False is NOT the contract: it drops the carried side mask between visits, for the test that shows the cases need it."""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    fb = np.zeros((cam.width * cam.height, 4), F)
    rays = vc.camera_rays(cam)
    rays["color"] = 0  # a camera ray starts with no colour, no opacity and no flags: it carries no side mask
    rays["w"] = 0
    rays["depth"] = 0
    if plane is not None:
        ids = rays["id"].astype(np.int64)
        inside = (ids >= 0) & (ids < cam.width * cam.height)
        t = np.where(inside, np.ascontiguousarray(plane, F).reshape(-1)[np.where(inside, ids, 0)], F(np.inf)).astype(F)
        rays["t_max"] = np.where(inside, t, rays["t_max"])
        with np.errstate(all="ignore"):
            rays["depth"] = np.where(t < F(np.inf), cc.CLIP, 0)
    brick = cc.next_brick(lo, hi, order, rays, -1)
    rays, brick = rays[brick >= 0], brick[brick >= 0]  # no first brick: dropped, nothing deposited
    visits = deposits = crossings = shaded = 0
    while len(rays):
        b = int(brick[0])  # one ray-set: the rays that are in brick b now
        here = brick == b
        visits += int(here.sum())
        out = lc.march(bricks[b], S, rays[here], minv, mode)
        crossings += lc.march.crossings
        shaded += lc.march.shaded
        opaque = (out["depth"] & vc.OPAQUE) != 0
        out["depth"] &= ~(vc.OPAQUE | vc.BOUNDARY)  # (SIDES and CLIP stay, and with them the mask in t)
        if not keep_sides:
            out["depth"] &= ~sc.SIDES
        nxt = np.full(len(out), -1, np.int64)
        if (~opaque).any():
            nxt[~opaque] = cc.next_brick(lo, hi, order, out[~opaque], b)
        done = nxt < 0  # OPAQUE, or EXTERNAL
        dep = out[done]
        ids = dep["id"].astype(np.int64)
        ok = (ids >= 0) & (ids < len(fb))
        np.add.at(fb, (ids[ok], slice(0, 3)), dep["color"][ok])
        np.add.at(fb, (ids[ok], 3), dep["w"][ok])
        deposits += int(done.sum())
        rays = np.concatenate([rays[~here], out[~done]])
        brick = np.concatenate([brick[~here], nxt[~done]])
    return fb.reshape(cam.height, cam.width, 4), {"brick_visits": visits, "rays_deposited": deposits, "crossings_rendered": crossings,
                                                 "samples_shaded": shaded}
