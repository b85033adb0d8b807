"""numpy restatement of the fused frame over AMR bricks (include/gvt_hip.h, "fused frame: AMR bricks"; gravit_amd/csrc/
volume_fused_amr.inc): tests/volume_fused_checker.py's order of work -- every camera ray followed from brick to brick until it deposits,
one ray-set at a time, no queues, no rounds -- over bricks of which some have subgrids and some have none.  The visit of a brick that
has subgrids is tests/volume_amr_checker.py's march (plain) or tests/volume_amr_surface_checker.py's (surfaces, lit fog); the visit of a
brick without is the existing checkers': tests/volume_clip_checker.py's march (plain) or tests/volume_shade_checker.py's.  Between two
visits only OPAQUE | BOUNDARY are cleared, as in tests/volume_fused_shaded_checker.py: the SIDES flag and the side mask in the ray's t
field stay, and so does t_min.  tests/test_volume_fused_amr_host.py shows that it gives the loop checkers' bits and visits."""
import numpy as np

from oracle import orc
from tests import volume_amr_checker as ac
from tests import volume_amr_surface_checker as asc
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_shade_checker as lc

F = np.float32


def frame(bricks, lo, hi, minv, cam, S=None, mode=lc.SHADE_NONE, plane=None):
    """gvt_hip_volume_frame_fused_amr over `bricks` (ac.AmrBrick; .sub empty: a brick without subgrids) with S and the mode on every
    brick (S None: the plain frame): the (H, W, 4) un-clamped framebuffer and the counts {brick_visits, rays_deposited, samples_refined,
    crossings, shaded, crossings_level (level -> crossings detected at samples of AMR bricks whose final grid has that level), plain_to_amr,
    amr_to_plain (ray transitions between a brick without and a brick with subgrids)}.  Like its parents it interpolates every sample,
    so samples_refined is the device's count without skipping.  plane: (H, W) floats (the clipped frame), or None."""
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
    has_sub = np.array([len(B.sub) > 0 for B in bricks], bool)
    brick = cc.next_brick(lo, hi, order, rays, -1)
    rays, brick = rays[brick >= 0], brick[brick >= 0]  # no first brick: dropped, nothing deposited
    n = {"brick_visits": 0, "rays_deposited": 0, "samples_refined": 0, "crossings": 0, "shaded": 0, "crossings_level": {}, "plain_to_amr": 0,
         "amr_to_plain": 0}
    while len(rays):
        b = int(brick[0])  # one ray-set: the rays that are in brick b now
        here = brick == b
        n["brick_visits"] += int(here.sum())
        B = bricks[b]
        if has_sub[b]:
            counts = {}
            if S is None:
                out = ac.march(B, rays[here], minv, counts)
            else:
                out = asc.march(B, S, rays[here], minv, mode, counts)
                n["crossings"] += counts["crossings"]
                n["shaded"] += counts["shaded"]
                for level, c in counts["crossings_level"].items():
                    n["crossings_level"][level] = n["crossings_level"].get(level, 0) + c
            n["samples_refined"] += counts["refined"]
        elif S is None:
            out = cc.march(B, rays[here], minv)
        else:
            out = lc.march(B, S, rays[here], minv, mode)
            n["crossings"] += lc.march.crossings
            n["shaded"] += lc.march.shaded
        opaque = (out["depth"] & vc.OPAQUE) != 0
        out["depth"] &= ~(vc.OPAQUE | vc.BOUNDARY)  # (SIDES and CLIP stay, and with them the mask in t)
        nxt = np.full(len(out), -1, np.int64)
        if (~opaque).any():
            nxt[~opaque] = cc.next_brick(lo, hi, order, out[~opaque], b)
        done = nxt < 0  # OPAQUE, or EXTERNAL
        to_amr = has_sub[np.maximum(nxt, 0)] & ~done
        n["plain_to_amr"] += 0 if has_sub[b] else int(to_amr.sum())
        n["amr_to_plain"] += int((~to_amr & ~done).sum()) if has_sub[b] else 0
        dep = out[done]
        ids = dep["id"].astype(np.int64)
        ok = (ids >= 0) & (ids < len(fb))
        np.add.at(fb, (ids[ok], slice(0, 3)), dep["color"][ok])
        np.add.at(fb, (ids[ok], 3), dep["w"][ok])
        n["rays_deposited"] += int(done.sum())
        rays = np.concatenate([rays[~here], out[~done]])
        brick = np.concatenate([brick[~here], nxt[~done]])
    return fb.reshape(cam.height, cam.width, 4), n
