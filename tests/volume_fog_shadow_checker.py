"""numpy float32 restatement of SHADOWED FOG (include/gvt_hip.h, "shadowed fog"; gravit_amd/csrc/volume_light_grid.inc and
volume_fused_fog.inc), on top of tests/volume_shadow_checker.py.

grid()   G_j at every global vertex: the shadow ray from the vertex (p = origin + (float)I * spacing, wp = m applied as a point) towards
         light j, t_min = (float)(bias - 1) * dt, walked with volume_shadow_checker.shadow_opacity over the WHOLE grid as ONE brick;
         G = 1 - A_s.  That is the definition: the device must give these bits for every bricking.
frame()  volume_shadow_checker.frame -- crossings lit through exact shadow rays -- in which a shaded lit fog sample multiplies each
         light's n . l by Tg, the trilinear interpolation of G_j at the eight vertices of the sample's cell (the sample's fractions, the
         value's nesting: x, then y, then z).  Without surfaces no crossing exists and the first two steps of that frame fall away.
march() restates volume_shadow_checker.march for that one change."""
import numpy as np

from oracle import orc
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_shade_checker as lc
from tests import volume_shadow_checker as sw
from tests import volume_surface_checker as sc

F = np.float32


def vertex_points(B, m):
    """(object-space p, world-space wp) of every vertex of brick B, x fastest: p = go + (float)(off + i) * sp, wp = xfm_point(m, p)."""
    nx, ny, nz = (int(v) for v in B.n)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    I = np.stack([i.reshape(-1), j.reshape(-1), k.reshape(-1)], axis=1) + B.off[None, :]
    p = (B.go[None, :] + I.astype(F) * B.sp[None, :]).astype(F)
    return p, vc.xfm_point(m, p)


def opacity(bricks, lo, hi, m, minv, S, origin_brick, direction, bias=1):
    """A_s of the rays from the vertices of origin_brick towards `direction` (world space, unit), walked over `bricks` by the EXISTING
    next-brick walk (volume_shadow_checker.shadow_opacity): over one brick the definition, over several the walk the finding is about."""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    _, wp = vertex_points(origin_brick, m)
    t_min = F(bias - 1) * bricks[0].dt
    return sw.shadow_opacity(bricks, lo, hi, order, minv, S, wp, np.broadcast_to(np.asarray(direction, F), wp.shape), t_min)[0]


def opacity_owned(bricks, whole, m, minv, S, direction, bias=1):
    """A_s of the same rays walked over `bricks` the way the bake walks them, by SAMPLE OWNERSHIP: the lattice range once from the global
    vertex box; the next visit goes to the brick that owns the global cell of the first lattice index after t_min (before the ray's
    first sample, indices outside the grid are passed over); the visit is volume_shade_checker.march's, which ends by the contiguity
    rule; the ray ends when that cell lies outside the grid or when A >= OPAQUE_A.  The side mask travels in the ray, as ever."""
    from gravit_amd.layouts import RAY_DTYPE

    _, wp = vertex_points(whole, m)
    n = len(wp)
    rays = np.zeros(n, RAY_DTYPE)
    rays["origin"], rays["direction"] = wp, np.broadcast_to(np.asarray(direction, F), wp.shape)
    rays["t_min"] = F(bias - 1) * whole.dt
    rays["t_max"] = np.inf
    rays["id"] = np.arange(n)
    o, d = vc.xfm_point(minv, rays["origin"]), vc.xfm_vector(minv, rays["direction"])
    # the one brick's range (volume_shade_checker.march's expressions on the global box)
    tn, tf = vc.slab(whole.lo, whole.hi, o, d)
    kp = vc.first_after(rays["t_min"], whole.dt)
    with np.errstate(all="ignore"):
        qlo, qhi = np.floor(tn / whole.dt), np.floor(tf / whole.dt)
        ok = (tn <= tf) & (tf >= 0) & (tf < np.inf) & (kp >= 0) & (qlo < vc.K_MAX)
        kb = np.where(qlo > 1, np.nan_to_num(qlo, neginf=0, posinf=0).astype(np.int64) - 1, 0)
        qh = np.nan_to_num(qhi, neginf=0, posinf=0).astype(np.int64)
    k = np.where(ok, np.maximum(kp, kb), 0)
    k_hi = np.where(ok, np.where(qhi < vc.K_MAX, qh + 1, int(vc.K_MAX)), -1)
    k_hi = np.where(ok, np.minimum(k_hi, k + vc.MAX_SAMPLES), k_hi)
    A = np.zeros(n, F)
    seen = np.zeros(n, bool)
    live = np.nonzero(k <= k_hi)[0]
    while len(live):
        inside = vc.cells(whole, o[live], d[live], k[live])[0]
        over = ~inside & seen[live]  # the first index after the last sample lies outside the grid: the ray is over
        k[live[~inside & ~seen[live]]] += 1  # nothing seen yet: the next index
        live = live[~over]
        live = live[k[live] <= k_hi[live]]
        go = live[vc.cells(whole, o[live], d[live], k[live])[0]]
        if not len(go):
            continue
        _, gc, _ = vc.cells(whole, o[go], d[go], k[go])
        owner = np.full(len(go), -1, np.int64)
        for b, B in enumerate(bricks):
            owner[np.all((gc >= B.off) & (gc <= B.off + B.n - 2), axis=1)] = b
        assert (owner >= 0).all()  # the bricks tile the grid
        for b in np.unique(owner):
            idx = go[owner == b]
            out = lc.march(bricks[b], S, rays[idx], minv, lc.SHADE_NONE)
            assert (np.round(out["t_min"] / whole.dt) >= k[idx]).all()  # every visit owns at least one sample: sample k
            out["depth"] &= ~(vc.OPAQUE | vc.BOUNDARY)
            rays[idx] = out
            A[idx] = out["w"]
            seen[idx] = True
            k[idx] = vc.first_after(out["t_min"], whole.dt)
        live = live[(A[live] < vc.OPAQUE_A) & (k[live] <= k_hi[live])]
    return A


def grid(whole, lo, hi, m, minv, S, bias=1):
    """(G (lights, gz, gy, gx) float32 with 1 for a light that casts no ray, usable (lights,) bool).  whole: the vc.Brick of the whole
    grid (offset 0), lo / hi its world box."""
    ws, usable = sw.light_rays(S)
    nx, ny, nz = (int(v) for v in whole.n)
    G = np.ones((len(ws), nz, ny, nx), F)
    for j in np.nonzero(usable)[0]:
        A_s = opacity([whole], lo, hi, m, minv, S, whole, ws[j], bias)
        G[j] = (F(1) - A_s).astype(F).reshape(nz, ny, nx)
    return G, usable


def brick_grid(G, B):
    """The part of G a brick stores: its own vertices."""
    o, n = B.off, B.n
    return G[:, o[2]:o[2] + n[2], o[1]:o[1] + n[1], o[0]:o[0] + n[0]]


def shade(S, ldir, rgba, g, Tg):
    """volume_shade_checker.shade with Tg (n, lights): ndl_s = ndl * Tg."""
    with np.errstate(all="ignore"):
        shaded = rgba[:, 3] > 0
        ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F)
        ok = (ln > 0) & (ln < np.inf)
        nrm = (g / np.where(ok, ln, F(1))[:, None]).astype(F)
        tot = np.zeros((len(g), 3), F)
        for j in range(len(ldir)):
            ndl = np.abs((nrm[:, 0] * ldir[j, 0] + nrm[:, 1] * ldir[j, 1]) + nrm[:, 2] * ldir[j, 2]).astype(F)
            ndl_s = (ndl * Tg[:, j]).astype(F)
            tot = (tot + S.lcol[j][None, :] * ndl_s[:, None]).astype(F)
        tot = np.where(ok[:, None], tot, F(0))
        lit = (rgba[:, :3] * (S.ka + S.kd * tot)).astype(F)
        return np.where(shaded[:, None], lit, rgba[:, :3]).astype(F), shaded


def march(B, S, rays, minv, mode, T, events, G):
    """volume_shadow_checker.march with the light grids: G (lights, gz, gy, gx) of the WHOLE grid (a brick reads its own part of it), or
    None for a frame whose fog is not shadowed.  T / events: as there (both None: no surfaces, so no crossing is ever rendered)."""
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
    gflat = None if G is None else np.ascontiguousarray(brick_grid(G, B)).reshape(n_lights, -1)
    crossings = n_shaded = 0
    shaded_ids = []
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
                Cj[sel], Aj[sel] = sw.composite(S, ldir, col, g, Cj[sel], Aj[sel], Tj[sel])
            stop = (crossed != 0) & (Aj >= vc.OPAQUE_A)  # the surface ends the ray: the sample itself adds nothing
            rgba = sc.lookup(B, v)
            rgb = rgba[:, :3]
            if lit:
                Tg = np.ones((len(j), n_lights), F)
                if gflat is not None:  # the grids at the cell's vertices, interpolated like the value
                    for l in range(n_lights):
                        g000, g100, g010, g110, g001, g101, g011, g111 = (gflat[l][a] for a in at)
                        a00, a10 = vc.lerp(g000, g100, fx), vc.lerp(g010, g110, fx)
                        a01, a11 = vc.lerp(g001, g101, fx), vc.lerp(g011, g111, fx)
                        Tg[:, l] = vc.lerp(vc.lerp(a00, a10, fy), vc.lerp(a01, a11, fy), fz)
                rgb, shaded = shade(S, ldir, rgba, g_cell, Tg)
                n_shaded += int((shaded & ~stop).sum())
                shaded_ids.append(r["id"][j[shaded & ~stop]].astype(np.int64))
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
    march.shaded_ids = np.unique(np.concatenate(shaded_ids)) if shaded_ids else np.zeros(0, np.int64)
    return r


def _walk(bricks, lo, hi, order, minv, cam, S, mode, plane, T, events, G):
    """volume_shadow_checker._walk around the march above."""
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
    shaded_pixels = np.zeros(len(fb), bool)
    while len(rays):
        b = int(brick[0])
        here = brick == b
        visits += int(here.sum())
        out = march(bricks[b], S, rays[here], minv, mode, T, events, G)
        crossings += march.crossings
        shaded += march.shaded
        ids = march.shaded_ids
        shaded_pixels[ids[(ids >= 0) & (ids < len(fb))]] = True
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
                                                 "samples_shaded": shaded, "shaded_pixels": shaded_pixels}


def frame(bricks, lo, hi, minv, cam, S, mode, G, plane=None, bias=2):
    """gvt_hip_volume_frame_fog_shadowed with S (lights; surfaces or none) and the mode on every brick, G = grid()'s first result (None:
    the fog unshadowed -- gvt_hip_volume_frame_shadowed, or without surfaces the shaded fused frame): the (H, W, 4) un-clamped
    framebuffer and the counters of volume_shadow_checker.frame (the shadow rays' are 0 without surfaces), with "shaded_pixels": per
    pixel of the film, does its ray shade a fog sample?"""
    assert len(S.lpos) and 1 <= bias <= 64
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    T = None
    extra = {"shadow_rays": 0, "shadow_brick_visits": 0, "shadow_crossings": 0}
    if len(S):
        events = []
        _walk(bricks, lo, hi, order, minv, cam, S, mode, plane, None, events, None)  # (opacity never depends on colour: the samples are the same)
        ids = np.concatenate([e[0] for e in events]) if events else np.zeros(0, np.int64)
        ks = np.concatenate([e[1] for e in events]) if events else np.zeros(0, np.int64)
        wp = np.concatenate([e[2] for e in events]) if events else np.zeros((0, 3), F)
        ws, usable = sw.light_rays(S)
        A_s = np.zeros((len(ids), len(ws)), F)
        t_min = F(bias - 1) * bricks[0].dt
        for j in np.nonzero(usable)[0]:
            A_s[:, j], v, c = sw.shadow_opacity(bricks, lo, hi, order, minv, S, wp, np.broadcast_to(ws[j], wp.shape), t_min)
            extra["shadow_brick_visits"] += v
            extra["shadow_crossings"] += c
        extra["shadow_rays"] = len(ids) * int(usable.sum())
        T = sw.Transmittance(sw._keys(ids, ks), (F(1) - A_s).astype(F))
    fb, counters = _walk(bricks, lo, hi, order, minv, cam, S, mode, plane, T, None, G)
    counters.update(extra)
    return fb, counters
