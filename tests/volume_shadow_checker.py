"""numpy float32 restatement of SHADOWED SURFACES (include/gvt_hip.h, "shadowed surfaces"; gravit_amd/csrc/volume_fused_shadow.inc):
tests/volume_fused_shaded_checker.py's per-ray walk -- every camera ray followed from brick to brick until it deposits -- around
tests/volume_shade_checker.py's march, restated here because the composite of a crossing takes a transmittance per light:

    ndl_s = ndl * T_j;  sum = sum + lcol_j * ndl_s

T_j is defined by reduction to the contract that exists: T_j = 1 - A_s, A_s the opacity the shadow ray deposits as a camera ray of the
shaded fused frame with shading NONE.  So the shadow rays are walked with volume_shade_checker.march itself in mode NONE, and `w` is read.

Opacity never depends on colour, so the samples at which a camera ray renders a crossing are those of the unshadowed frame.  The frame is
therefore computed in three steps: the walk once with every T = 1, recording each (ray, sample) with a rendered crossing and the world
point wp = wo + wd * ((float)k * dt); ONE walk of all their shadow rays; the walk again with the T found."""
import numpy as np

from gravit_amd.layouts import RAY_DTYPE
from oracle import orc
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_shade_checker as lc
from tests import volume_surface_checker as sc

F = np.float32


def light_rays(S):
    """ws_j = lpos_j / sqrt((x*x + y*y) + z*z) in float32, world space, towards the light; usable: neither zero nor not finite."""
    lp = S.lpos.astype(F)
    with np.errstate(all="ignore"):
        ln = np.sqrt((lp[:, 0] * lp[:, 0] + lp[:, 1] * lp[:, 1]) + lp[:, 2] * lp[:, 2]).astype(F)
        ok = (ln > 0) & np.isfinite(ln)
        ws = np.where(ok[:, None], lp / np.where(ok, ln, F(1))[:, None], F(0)).astype(F)
    return ws, ok


def composite(S, ldir, c, g, C, A, T):
    """volume_surface_checker.composite with T (n, lights): the one changed line of the contract."""
    with np.errstate(all="ignore"):
        ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F)
        ok = ln > 0
        nrm = (g / np.where(ok, ln, F(1))[:, None]).astype(F)
        tot = np.zeros_like(c)
        for j in range(len(ldir)):
            ndl = np.abs((nrm[:, 0] * ldir[j, 0] + nrm[:, 1] * ldir[j, 1]) + nrm[:, 2] * ldir[j, 2]).astype(F)
            ndl_s = (ndl * T[:, j]).astype(F)
            tot = (tot + S.lcol[j][None, :] * ndl_s[:, None]).astype(F)
        tot = np.where(ok[:, None], tot, F(0))
        rgb = (c * (S.ka + S.kd * tot)).astype(F)
        f = ((F(1) - A) * S.opacity).astype(F)
        return (C + f[:, None] * rgb).astype(F), (A + f).astype(F)


def _keys(ids, k):
    return (np.asarray(ids, np.int64) << 32) | np.asarray(k, np.int64)


class Transmittance:
    """T per (camera ray, sample): rows found by key (pixel id, k).  None in its place: every T = 1, and the samples are recorded."""

    def __init__(self, keys, T):
        order = np.argsort(keys)
        self.keys, self.T = keys[order], T[order]

    def rows(self, ids, k):
        want = _keys(ids, k)
        at = np.searchsorted(self.keys, want)
        assert (at < len(self.keys)).all() and (self.keys[np.minimum(at, len(self.keys) - 1)] == want).all()  # the second walk meets the first's samples
        return self.T[at]


def march(B, S, rays, minv, mode, T, events):
    """volume_shade_checker.march (S has surfaces and lights) with the transmittances: T a Transmittance, or None for the recording pass,
    which appends (ids, k, wp) of every sample with a rendered crossing to events."""
    n_surf = len(S)
    lit = mode == lc.SHADE_GRADIENT and len(S.lpos) > 0
    n_lights = len(S.lpos)
    r = rays.copy()
    o = vc.xfm_point(minv, r["origin"])
    d = vc.xfm_vector(minv, r["direction"])
    n = len(r)
    C = r["color"].astype(F).copy()
    A = r["w"].astype(F).copy()
    tn, tf = vc.slab(B.lo, B.hi, o, d)
    kp = vc.first_after(r["t_min"], B.dt)
    with np.errstate(all="ignore"):
        qlo, qhi = np.floor(tn / B.dt), np.floor(tf / B.dt)
        ok = (tn <= tf) & (tf >= 0) & (tf < np.inf) & (kp >= 0) & (qlo < vc.K_MAX)
        kb = np.where(qlo > 1, np.nan_to_num(qlo, neginf=0, posinf=0).astype(np.int64) - 1, 0)
        qh = np.nan_to_num(qhi, neginf=0, posinf=0).astype(np.int64)
    k = np.where(ok, np.maximum(kp, kb), 0)
    k_hi = np.where(ok, np.where(qhi < vc.K_MAX, qh + 1, int(vc.K_MAX)), -1)
    k_hi = np.where(ok, np.minimum(k_hi, k + vc.MAX_SAMPLES), k_hi)
    flagged = (r["depth"] & cc.CLIP) != 0
    k_hi = np.where(ok & flagged, np.minimum(k_hi, cc.last_before(r["t_max"], B.dt)), k_hi)  # the clip, last
    k_last = np.full(n, -1, np.int64)
    seen = np.zeros(n, bool)
    carried = (r["depth"] & sc.SIDES) != 0
    with np.errstate(all="ignore"):
        prev = np.where(carried, np.nan_to_num(r["t"]).astype(np.int64) & 0xFFFF, -1)
    k_carry = np.where(carried, kp, -1)
    ldir = S.light_dirs(minv)
    n_iso = len(S.iso)
    active = k <= k_hi
    nx, ny = int(B.n[0]), int(B.n[1])
    flat = B.vox.reshape(-1)
    crossings = n_shaded = 0
    while True:
        act = np.nonzero(active)[0]
        if not len(act):
            break
        over = k[act] > k_hi[act]
        active[act[over]] = False
        act = act[~over]
        if not len(act):
            continue
        own, c, f = vc.cells(B, o[act], d[act], k[act])
        active[act[~own & seen[act]]] = False
        k[act[~own & ~seen[act]]] += 1
        j = act[own]
        if not len(j):
            continue
        c, f = c[own], f[own]
        first = ~seen[j]
        prev[j[first & (k[j] != k_carry[j])]] = -1
        seen[j] = True
        k_last[j] = k[j]
        t = k[j].astype(F) * B.dt
        p = (o[j] + d[j] * t[:, None]).astype(F)
        base = c[:, 0] + nx * c[:, 1] + nx * ny * c[:, 2]
        sy, sz = nx, nx * ny
        v8 = (flat[base], flat[base + 1], flat[base + sy], flat[base + sy + 1],
              flat[base + sz], flat[base + sz + 1], flat[base + sz + sy], flat[base + sz + sy + 1])
        v000, v100, v010, v110, v001, v101, v011, v111 = v8
        fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
        with np.errstate(all="ignore"):
            c00, c10 = vc.lerp(v000, v100, fx), vc.lerp(v010, v110, fx)
            c01, c11 = vc.lerp(v001, v101, fx), vc.lerp(v011, v111, fx)
            c0, c1 = vc.lerp(c00, c10, fy), vc.lerp(c01, c11, fy)
            v = vc.lerp(c0, c1, fz)
            g_cell = lc.gradient(B, v8, fx, fy, fz) if lit or n_iso else None
            Cj, Aj = C[j], A[j]
            sides = np.zeros(len(j), np.int64)
            for i in range(n_iso):
                sides |= (v >= S.iso[i]).astype(np.int64) << i
            for i, P in enumerate(S.planes):
                sides |= (((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) >= P[3]).astype(np.int64) << (n_iso + i)
            crossed = np.where(prev[j] < 0, 0, sides ^ prev[j])
            prev[j] = sides
            hit = (crossed != 0) & (Aj < vc.OPAQUE_A)  # at least one crossing is rendered: the T_j of this sample, shared by its crossings
            Tj = np.ones((len(j), n_lights), F)
            if hit.any():
                if T is None:
                    wp = (r["origin"][j[hit]].astype(F) + r["direction"][j[hit]].astype(F) * t[hit][:, None]).astype(F)  # vol_point's form on the world ray
                    events.append((r["id"][j[hit]].astype(np.int64), k[j[hit]].copy(), wp))
                else:
                    Tj[hit] = T.rows(r["id"][j[hit]], k[j[hit]])
            for i in range(n_surf):
                sel = ((crossed >> i) & 1).astype(bool) & (Aj < vc.OPAQUE_A)
                if not sel.any():
                    continue
                crossings += int(sel.sum())
                if i < n_iso:
                    col = sc.lookup(B, np.full(int(sel.sum()), S.iso[i], F))[:, :3]
                    g = g_cell[sel]
                else:
                    col = sc.lookup(B, v[sel])[:, :3]
                    g = np.broadcast_to(S.planes[i - n_iso][:3], (int(sel.sum()), 3)).astype(F)
                Cj[sel], Aj[sel] = composite(S, ldir, col, g, Cj[sel], Aj[sel], Tj[sel])
            stop = (crossed != 0) & (Aj >= vc.OPAQUE_A)  # the surface ends the ray: the sample itself adds nothing
            rgba = sc.lookup(B, v)
            rgb = rgba[:, :3]
            if lit:  # the fog is lit as before and not shadowed
                rgb, shaded = lc.shade(S, ldir, rgba, g_cell)
                n_shaded += int((shaded & ~stop).sum())
            fr = ((F(1) - Aj) * rgba[:, 3]).astype(F)
            Cn = (Cj + fr[:, None] * rgb).astype(F)
            An = (Aj + fr).astype(F)
        C[j] = np.where(stop[:, None], Cj, Cn)
        A[j] = np.where(stop, Aj, An)
        k[j] += 1
        active[j[A[j] >= vc.OPAQUE_A]] = False
    marched = k_last >= 0
    r["t_min"] = np.where(marched, k_last.astype(F) * B.dt, r["t_min"])
    r["color"] = C
    r["w"] = A
    r["depth"] = r["depth"] | np.where(A >= vc.OPAQUE_A, vc.OPAQUE, vc.BOUNDARY).astype(np.int32)
    r["t"] = np.where(marched, prev.astype(F), r["t"])
    r["depth"] = r["depth"] | np.where(marched, sc.SIDES, 0).astype(np.int32)
    march.crossings, march.shaded = crossings, n_shaded
    return r


def _walk(bricks, lo, hi, order, minv, cam, S, mode, plane, T, events):
    """volume_fused_shaded_checker.frame's walk around the march above."""
    fb = np.zeros((cam.width * cam.height, 4), F)
    rays = vc.camera_rays(cam)
    assert len(np.unique(rays["id"])) == len(rays)  # one ray per pixel: (id, k) names a sample
    rays["color"] = 0
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
    rays, brick = rays[brick >= 0], brick[brick >= 0]
    visits = deposits = crossings = shaded = 0
    while len(rays):
        b = int(brick[0])
        here = brick == b
        visits += int(here.sum())
        out = march(bricks[b], S, rays[here], minv, mode, T, events)
        crossings += march.crossings
        shaded += march.shaded
        opaque = (out["depth"] & vc.OPAQUE) != 0
        out["depth"] &= ~(vc.OPAQUE | vc.BOUNDARY)
        nxt = np.full(len(out), -1, np.int64)
        if (~opaque).any():
            nxt[~opaque] = cc.next_brick(lo, hi, order, out[~opaque], b)
        done = nxt < 0
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


def shadow_opacity(bricks, lo, hi, order, minv, S, origin, direction, t_min):
    """A_s of the shadow rays (origin (n, 3), direction (n, 3), world space): camera rays of the shaded fused frame with shading NONE -- no
    colour, no opacity, no flags, no clip -- walked with volume_shade_checker.march; w is read where a ray ends.  A ray that meets no
    brick has A_s = 0.  Returns (A_s, brick visits, crossings rendered)."""
    n = len(origin)
    rays = np.zeros(n, RAY_DTYPE)
    rays["origin"], rays["direction"] = origin, direction
    rays["t_min"] = t_min
    rays["t_max"] = np.inf
    rays["id"] = np.arange(n)
    A = np.zeros(n, F)
    brick = cc.next_brick(lo, hi, order, rays, -1)
    rays, brick = rays[brick >= 0], brick[brick >= 0]
    visits = crossings = 0
    while len(rays):
        b = int(brick[0])
        here = brick == b
        visits += int(here.sum())
        out = lc.march(bricks[b], S, rays[here], minv, lc.SHADE_NONE)
        crossings += lc.march.crossings
        opaque = (out["depth"] & vc.OPAQUE) != 0
        out["depth"] &= ~(vc.OPAQUE | vc.BOUNDARY)
        nxt = np.full(len(out), -1, np.int64)
        if (~opaque).any():
            nxt[~opaque] = cc.next_brick(lo, hi, order, out[~opaque], b)
        done = nxt < 0
        A[out["id"][done]] = out["w"][done]
        rays = np.concatenate([rays[~here], out[~done]])
        brick = np.concatenate([brick[~here], nxt[~done]])
    return A, visits, crossings


def frame(bricks, lo, hi, minv, cam, S, mode=lc.SHADE_NONE, plane=None, bias=2):
    """gvt_hip_volume_frame_shadowed with S (surfaces and at least one light) and the mode on every brick: the (H, W, 4) un-clamped
    framebuffer, the counters of volume_fused_shaded_checker.frame plus {shadow_rays, shadow_brick_visits, shadow_crossings}, and
    details = {"ids", "k": the samples with a rendered crossing, "A_s": (samples, lights) the shadow rays' opacities (0 where a light
    casts none), "usable": per light}."""
    assert len(S) and len(S.lpos) and 1 <= bias <= 64
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    events = []
    _walk(bricks, lo, hi, order, minv, cam, S, mode, plane, None, events)
    ids = np.concatenate([e[0] for e in events]) if events else np.zeros(0, np.int64)
    ks = np.concatenate([e[1] for e in events]) if events else np.zeros(0, np.int64)
    wp = np.concatenate([e[2] for e in events]) if events else np.zeros((0, 3), F)
    ws, usable = light_rays(S)
    A_s = np.zeros((len(ids), len(ws)), F)
    t_min = F(bias - 1) * bricks[0].dt
    s_visits = s_crossings = 0
    for j in np.nonzero(usable)[0]:
        A_s[:, j], v, c = shadow_opacity(bricks, lo, hi, order, minv, S, wp, np.broadcast_to(ws[j], wp.shape), t_min)
        s_visits += v
        s_crossings += c
    T = Transmittance(_keys(ids, ks), (F(1) - A_s).astype(F))
    fb, counters = _walk(bricks, lo, hi, order, minv, cam, S, mode, plane, T, None)
    counters.update(shadow_rays=len(ids) * int(usable.sum()), shadow_brick_visits=s_visits, shadow_crossings=s_crossings)
    return fb, counters, {"ids": ids, "k": ks, "A_s": A_s, "usable": usable}
