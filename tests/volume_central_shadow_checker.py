"""numpy float32 restatement of the SHADOWED FRAMES WITH A GRADIENT KIND (include/gvt_hip.h, "shadowed surfaces", CENTRAL; the CENTRAL
instantiations of gravit_amd/csrc/volume_fused_shadow.inc, volume_fused_fog.inc and volume_fused_mesh.inc): ONE march that takes

    kind   CELL or CENTRAL: the g that shades a crossed isovalue and a lit fog sample (volume_smooth_checker.central_gradient for CENTRAL,
           on volume_smooth_checker.Brick, which carries the ghost layers);
    T      a volume_shadow_checker.Transmittance per (camera ray, sample with a rendered crossing), or None for the pass that records
           those samples (every T = 1);
    G      the light grids of volume_fog_shadow_checker.grid (or None: the fog is not shadowed);
    O      the occluder grids of volume_mesh_shadow_checker.occluders (or None: no mesh shadows the volume);

and frame() around it.  T, G and O come from the existing checkers' functions unchanged: none of them reads a gradient -- the shadow rays
and the bakes march with shading NONE -- so T_j, Tg, Og, the counters and the opacity are those of the same frame under CELL.  With kind
CELL the frames here are volume_shadow_checker.frame, volume_fog_shadow_checker.frame and volume_mesh_shadow_checker.frame bit for bit;
with CENTRAL and no shadows, volume_smooth_checker.frame(kind=CENTRAL) (tests/test_volume_fused_central_host.py pins both ends)."""
import numpy as np

from oracle import orc
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_fog_shadow_checker as fg
from tests import volume_shade_checker as lc
from tests import volume_shadow_checker as sw
from tests import volume_smooth_checker as sm
from tests import volume_surface_checker as sc

F = np.float32
CELL, CENTRAL = sm.CELL, sm.CENTRAL


def _lerp8(flat, at, fx, fy, fz):
    """the trilinear interpolation of a plane at the cell's eight vertices, the value's nesting: x, then y, then z"""
    a000, a100, a010, a110, a001, a101, a011, a111 = (flat[a] for a in at)
    a00, a10 = vc.lerp(a000, a100, fx), vc.lerp(a010, a110, fx)
    a01, a11 = vc.lerp(a001, a101, fx), vc.lerp(a011, a111, fx)
    return vc.lerp(vc.lerp(a00, a10, fy), vc.lerp(a01, a11, fy), fz)


def march(B, S, rays, minv, mode, kind, T, events, G=None, O=None):
    """One visit of brick B (a volume_smooth_checker.Brick for CENTRAL) by `rays`: the surface / lit march with a transmittance per light
    at every crossing (T, times Og where O is given) and at every lit fog sample (Tg from G, times Og), shaded by the gradient of `kind`.
    T None: the recording pass, which appends (ids, k, wp) of every sample with a rendered crossing to events (None: nothing is kept)."""
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
    gflat = None if G is None else np.ascontiguousarray(fg.brick_grid(G, B)).reshape(n_lights, -1)
    oflat = None if O is None else np.ascontiguousarray(fg.brick_grid(O, B)).astype(F).reshape(n_lights, -1)  # ((float)O is exact)
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
        at = (base, base + 1, base + sy, base + sy + 1, base + sz, base + sz + 1, base + sz + sy, base + sz + sy + 1)
        v8 = tuple(flat[a] for a in at)
        v000, v100, v010, v110, v001, v101, v011, v111 = v8
        fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
        with np.errstate(all="ignore"):
            c00, c10 = vc.lerp(v000, v100, fx), vc.lerp(v010, v110, fx)
            c01, c11 = vc.lerp(v001, v101, fx), vc.lerp(v011, v111, fx)
            c0, c1 = vc.lerp(c00, c10, fy), vc.lerp(c01, c11, fy)
            v = vc.lerp(c0, c1, fz)
            g_shade = None  # the contract's one change: the kind's gradient
            if lit or n_iso:
                g_shade = sm.central_gradient(B, c, fx, fy, fz) if kind == CENTRAL else lc.gradient(B, v8, fx, fy, fz)
            Cj, Aj = C[j], A[j]
            sides = np.zeros(len(j), np.int64)
            for i in range(n_iso):
                sides |= (v >= S.iso[i]).astype(np.int64) << i
            for i, P in enumerate(S.planes):
                sides |= (((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) >= P[3]).astype(np.int64) << (n_iso + i)
            crossed = np.where(prev[j] < 0, 0, sides ^ prev[j])
            prev[j] = sides
            hit = (crossed != 0) & (Aj < vc.OPAQUE_A)  # at least one crossing is rendered: the T_j of this sample, shared by its crossings
            Og = None
            if oflat is not None:
                Og = np.ones((len(j), n_lights), F)
                for l in range(n_lights):
                    Og[:, l] = _lerp8(oflat[l], at, fx, fy, fz)
            Tj = np.ones((len(j), n_lights), F)
            if hit.any():
                if T is None:
                    if events is not None:
                        wp = (r["origin"][j[hit]].astype(F) + r["direction"][j[hit]].astype(F) * t[hit][:, None]).astype(F)  # vol_point's form on the world ray
                        events.append((r["id"][j[hit]].astype(np.int64), k[j[hit]].copy(), wp))
                else:
                    Tj[hit] = T.rows(r["id"][j[hit]], k[j[hit]])
                    if Og is not None:
                        Tj[hit] = (Tj[hit] * Og[hit]).astype(F)  # T_j * Og, once for all the sample's crossings
            for i in range(n_surf):
                sel = ((crossed >> i) & 1).astype(bool) & (Aj < vc.OPAQUE_A)
                if not sel.any():
                    continue
                crossings += int(sel.sum())
                if i < n_iso:
                    col = sc.lookup(B, np.full(int(sel.sum()), S.iso[i], F))[:, :3]
                    g = g_shade[sel]
                else:
                    col = sc.lookup(B, v[sel])[:, :3]
                    g = np.broadcast_to(S.planes[i - n_iso][:3], (int(sel.sum()), 3)).astype(F)
                Cj[sel], Aj[sel] = sw.composite(S, ldir, col, g, Cj[sel], Aj[sel], Tj[sel])
            stop = (crossed != 0) & (Aj >= vc.OPAQUE_A)  # the surface ends the ray: the sample itself adds nothing
            rgba = sc.lookup(B, v)
            rgb = rgba[:, :3]
            if lit:
                Ts = np.ones((len(j), n_lights), F)
                if gflat is not None:
                    for l in range(n_lights):
                        Ts[:, l] = _lerp8(gflat[l], at, fx, fy, fz)
                if Og is not None:
                    Ts = (Ts * Og).astype(F)
                rgb, shaded = fg.shade(S, ldir, rgba, g_shade, Ts)
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


def _walk(bricks, lo, hi, order, minv, cam, S, mode, kind, plane, T, events, G, O):
    """The fused frame's walk -- every camera ray followed from brick to brick until it deposits -- around the march above."""
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
        out = march(bricks[b], S, rays[here], minv, mode, kind, T, events, G, O)
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


def frame(bricks, lo, hi, minv, cam, S, mode=lc.SHADE_NONE, kind=CELL, G=None, O=None, plane=None, bias=2, shadows=True):
    """The shadowed frames with S (lights; surfaces or none), the mode and the gradient kind on every brick: G None and O None is
    gvt_hip_volume_frame_shadowed, G alone gvt_hip_volume_frame_fog_shadowed, O (with G where the fog is lit) gvt_hip_volume_frame_mesh_shadowed.
    shadows=False: every T = 1 (give no grids) -- the shaded fused frame, whose bits are the loop's.  Returns the (H, W, 4) un-clamped
    framebuffer and the counters of volume_shadow_checker.frame (the shadow rays' are 0 without surfaces or without shadows)."""
    assert len(S.lpos) and 1 <= bias <= 64
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    extra = {"shadow_rays": 0, "shadow_brick_visits": 0, "shadow_crossings": 0}
    if not shadows:
        assert G is None and O is None
        fb, counters = _walk(bricks, lo, hi, order, minv, cam, S, mode, kind, plane, None, None, None, None)
        counters.update(extra)
        return fb, counters
    T = None
    if len(S):
        events = []
        _walk(bricks, lo, hi, order, minv, cam, S, mode, kind, plane, None, events, None, O)  # (opacity never depends on colour: the samples are the same)
        ids = np.concatenate([e[0] for e in events]) if events else np.zeros(0, np.int64)
        ks = np.concatenate([e[1] for e in events]) if events else np.zeros(0, np.int64)
        wp = np.concatenate([e[2] for e in events]) if events else np.zeros((0, 3), F)
        ws, usable = sw.light_rays(S)
        A_s = np.zeros((len(ids), len(ws)), F)
        t_min = F(bias - 1) * bricks[0].dt
        for j in np.nonzero(usable)[0]:  # (the shadow rays read no gradient: the existing walk, unchanged)
            A_s[:, j], v, c = sw.shadow_opacity(bricks, lo, hi, order, minv, S, wp, np.broadcast_to(ws[j], wp.shape), t_min)
            extra["shadow_brick_visits"] += v
            extra["shadow_crossings"] += c
        extra["shadow_rays"] = len(ids) * int(usable.sum())
        T = sw.Transmittance(sw._keys(ids, ks), (F(1) - A_s).astype(F))
    fb, counters = _walk(bricks, lo, hi, order, minv, cam, S, mode, kind, plane, T, None, G, O)
    counters.update(extra)
    return fb, counters
