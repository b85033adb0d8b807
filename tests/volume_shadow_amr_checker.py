"""numpy float32 restatement of SHADOWS ON AMR BRICKS (include/gvt_hip.h, "shadows on AMR bricks"; gravit_amd/csrc/
volume_fused_shadow_amr.inc): the shadowed, fog-shadowed and mesh-shadowed frames and the light grid over bricks of which some have
subgrids (tests/volume_amr_checker.AmrBrick; .sub empty: a brick without).

march()           tests/volume_mesh_shadow_checker.py's march -- which is the fog-shadowed march where O is all ones and the shadowed march
                  where G is None as well -- with tests/volume_amr_surface_checker.py's visit: the value, the eight corners and the
                  fractions of a sample are the FINAL grid's after the descent, the gradient divides by the final grid's spacing; G and O
                  are read at the sample's LEVEL-0 cell with its level-0 fractions.
shadow_opacity()  tests/volume_shadow_checker.py's walk of the shadow rays, the visit of a brick with subgrids being
                  volume_amr_surface_checker.march in mode NONE (a camera ray of the fused AMR frame, shading NONE).
grid()            the light grid by definition: the whole volume with all its subgrids as ONE brick.
opacity_owned()   tests/volume_fog_shadow_checker.py's ownership walk over AMR bricks: what the bake does on several bricks.
frame()           the three frames: G None and O None the shadowed frame, O None the fog-shadowed frame.
Like its parents it interpolates every sample (no skipping).  tests/test_volume_shadow_amr_host.py ties it to them."""
import numpy as np

from gravit_amd.layouts import RAY_DTYPE
from oracle import orc
from tests import volume_amr_checker as ac
from tests import volume_amr_surface_checker as asc
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_fog_shadow_checker as fg
from tests import volume_shade_checker as lc
from tests import volume_shadow_checker as sw
from tests import volume_surface_checker as sc

F = np.float32


def _visit_none(B, S, rays, minv, counts=None):
    """One visit of shadow rays: shading NONE, the AMR visit on a brick with subgrids.  Returns (marched rays, crossings rendered)."""
    if len(B.sub):
        c = {}
        out = asc.march(B, S, rays, minv, lc.SHADE_NONE, c)
        if counts is not None:
            counts["refined"] = counts.get("refined", 0) + c["refined"]
        return out, c["crossings"]
    out = lc.march(B, S, rays, minv, lc.SHADE_NONE)
    return out, lc.march.crossings


def shadow_opacity(bricks, lo, hi, order, minv, S, origin, direction, t_min, counts=None):
    """volume_shadow_checker.shadow_opacity over AMR bricks.  counts (a dict) is added to: "refined" (shadow samples whose final grid is
    a subgrid) and "transitions" (shadow rays going from a brick with subgrids to one without, or back)."""
    n = len(origin)
    rays = np.zeros(n, RAY_DTYPE)
    rays["origin"], rays["direction"] = origin, direction
    rays["t_min"] = t_min
    rays["t_max"] = np.inf
    rays["id"] = np.arange(n)
    A = np.zeros(n, F)
    has_sub = np.array([len(B.sub) > 0 for B in bricks], bool)
    brick = cc.next_brick(lo, hi, order, rays, -1)
    rays, brick = rays[brick >= 0], brick[brick >= 0]
    visits = crossings = 0
    while len(rays):
        b = int(brick[0])
        here = brick == b
        visits += int(here.sum())
        out, c = _visit_none(bricks[b], S, rays[here], minv, counts)
        crossings += c
        opaque = (out["depth"] & vc.OPAQUE) != 0
        out["depth"] &= ~(vc.OPAQUE | vc.BOUNDARY)
        nxt = np.full(len(out), -1, np.int64)
        if (~opaque).any():
            nxt[~opaque] = cc.next_brick(lo, hi, order, out[~opaque], b)
        done = nxt < 0
        if counts is not None:
            counts["transitions"] = counts.get("transitions", 0) + int((~done & (has_sub[np.maximum(nxt, 0)] != has_sub[b])).sum())
        A[out["id"][done]] = out["w"][done]
        rays = np.concatenate([rays[~here], out[~done]])
        brick = np.concatenate([brick[~here], nxt[~done]])
    return A, visits, crossings


def grid(whole, lo, hi, m, minv, S, bias=1):
    """volume_fog_shadow_checker.grid for a whole volume that may have subgrids: (G (lights, gz, gy, gx), usable).  The definition: the
    rays start at the level-0 vertices and cross the ONE brick with all its subgrids."""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    ws, usable = sw.light_rays(S)
    nx, ny, nz = (int(v) for v in whole.n)
    _, wp = fg.vertex_points(whole, m)
    t_min = F(bias - 1) * whole.dt
    G = np.ones((len(ws), nz, ny, nx), F)
    for j in np.nonzero(usable)[0]:
        A_s = shadow_opacity([whole], lo, hi, order, minv, S, wp, np.broadcast_to(ws[j], wp.shape), t_min)[0]
        G[j] = (F(1) - A_s).astype(F).reshape(nz, ny, nx)
    return G, usable


def opacity_owned(bricks, whole, m, minv, S, direction, bias=1):
    """volume_fog_shadow_checker.opacity_owned with the AMR visit on bricks that have subgrids (whole: the level-0 grid as one brick; its
    subgrids are not read here)."""
    _, wp = fg.vertex_points(whole, m)
    n = len(wp)
    rays = np.zeros(n, RAY_DTYPE)
    rays["origin"], rays["direction"] = wp, np.broadcast_to(np.asarray(direction, F), wp.shape)
    rays["t_min"] = F(bias - 1) * whole.dt
    rays["t_max"] = np.inf
    rays["id"] = np.arange(n)
    o, d = vc.xfm_point(minv, rays["origin"]), vc.xfm_vector(minv, rays["direction"])
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
        over = ~inside & seen[live]
        k[live[~inside & ~seen[live]]] += 1
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
            out, _ = _visit_none(bricks[b], S, rays[idx], minv)
            assert (np.round(out["t_min"] / whole.dt) >= k[idx]).all()  # every visit owns at least one sample: sample k
            out["depth"] &= ~(vc.OPAQUE | vc.BOUNDARY)
            rays[idx] = out
            A[idx] = out["w"]
            seen[idx] = True
            k[idx] = vc.first_after(out["t_min"], whole.dt)
        live = live[(A[live] < vc.OPAQUE_A) & (k[live] <= k_hi[live])]
    return A


def grid_owned(bricks, whole, m, minv, S, bias=1):
    """The light grid as the bake walks it over `bricks`: (G, usable), grid()'s form."""
    ws, usable = sw.light_rays(S)
    nx, ny, nz = (int(v) for v in whole.n)
    G = np.ones((len(ws), nz, ny, nx), F)
    for j in np.nonzero(usable)[0]:
        G[j] = (F(1) - opacity_owned(bricks, whole, m, minv, S, ws[j], bias)).astype(F).reshape(nz, ny, nx)
    return G, usable


def _lerp8(flat, at, fx, fy, fz):
    a000, a100, a010, a110, a001, a101, a011, a111 = (flat[a] for a in at)
    a00, a10 = vc.lerp(a000, a100, fx), vc.lerp(a010, a110, fx)
    a01, a11 = vc.lerp(a001, a101, fx), vc.lerp(a011, a111, fx)
    return vc.lerp(vc.lerp(a00, a10, fy), vc.lerp(a01, a11, fy), fz)


def march(B, S, rays, minv, mode, T, events, G, O, counts=None):
    """volume_mesh_shadow_checker.march (O None: all ones; G None: the fog unshadowed) with the AMR visit.  counts (a dict) is added to:
    "refined" (samples whose final grid is a subgrid) and "crossings_refined" (rendered crossings at such samples)."""
    n_surf = len(S)
    lit = mode == lc.SHADE_GRADIENT and len(S.lpos) > 0
    n_lights = len(S.lpos)
    lev, rt = asc.levels(B)
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
    gflat = None if G is None else np.ascontiguousarray(fg.brick_grid(G, B)).reshape(n_lights, -1)
    oflat = None if O is None else np.ascontiguousarray(fg.brick_grid(O, B)).astype(F).reshape(n_lights, -1)  # ((float)O is exact)
    crossings = n_shaded = refined = crossings_refined = 0
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
        # the planes: the level-0 cell, the level-0 fractions
        base = c[:, 0] + nx * c[:, 1] + nx * ny * c[:, 2]
        sy, sz = nx, nx * ny
        at = (base, base + 1, base + sy, base + sy + 1, base + sz, base + sz + 1, base + sz + sy, base + sz + sy + 1)
        fx0, fy0, fz0 = f[:, 0], f[:, 1], f[:, 2]
        # the value and the gradient: the final grid's cell, the descended fractions
        grid_, ci, ff = ac.descend(B, c, f)
        fine = grid_ >= 0
        R = np.where(fine, rt[np.maximum(grid_, 0)] if len(rt) else 1, 1)
        refined += int(fine.sum())
        v8 = asc.corners(B, grid_, ci)
        v000, v100, v010, v110, v001, v101, v011, v111 = v8
        fx, fy, fz = ff[:, 0], ff[:, 1], ff[:, 2]
        with np.errstate(all="ignore"):
            c00, c10 = vc.lerp(v000, v100, fx), vc.lerp(v010, v110, fx)
            c01, c11 = vc.lerp(v001, v101, fx), vc.lerp(v011, v111, fx)
            c0, c1 = vc.lerp(c00, c10, fy), vc.lerp(c01, c11, fy)
            v = vc.lerp(c0, c1, fz)
            g_cell = asc.gradient(B, v8, ff, R) if lit or n_iso else None
            Cj, Aj = C[j], A[j]
            sides = np.zeros(len(j), np.int64)
            for i in range(n_iso):
                sides |= (v >= S.iso[i]).astype(np.int64) << i
            for i, P in enumerate(S.planes):
                sides |= (((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) >= P[3]).astype(np.int64) << (n_iso + i)
            crossed = np.where(prev[j] < 0, 0, sides ^ prev[j])
            prev[j] = sides
            hit = (crossed != 0) & (Aj < vc.OPAQUE_A)  # at least one crossing is rendered: the T_j of this sample, shared by its crossings
            Og = np.ones((len(j), n_lights), F)
            if oflat is not None:
                for l in range(n_lights):
                    Og[:, l] = _lerp8(oflat[l], at, fx0, fy0, fz0)
            Tj = np.ones((len(j), n_lights), F)
            if hit.any():
                if T is None:
                    wp = (r["origin"][j[hit]].astype(F) + r["direction"][j[hit]].astype(F) * t[hit][:, None]).astype(F)  # vol_point's form on the world ray
                    events.append((r["id"][j[hit]].astype(np.int64), k[j[hit]].copy(), wp))
                elif oflat is not None:
                    Tj[hit] = (T.rows(r["id"][j[hit]], k[j[hit]]) * Og[hit]).astype(F)  # T_j * Og, once for all the sample's crossings
                else:
                    Tj[hit] = T.rows(r["id"][j[hit]], k[j[hit]])
            for i in range(n_surf):
                sel = ((crossed >> i) & 1).astype(bool) & (Aj < vc.OPAQUE_A)
                if not sel.any():
                    continue
                crossings += int(sel.sum())
                crossings_refined += int((sel & fine).sum())
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
                if gflat is not None:
                    for l in range(n_lights):
                        Tg[:, l] = _lerp8(gflat[l], at, fx0, fy0, fz0)
                if oflat is not None:
                    Tg = (Tg * Og).astype(F)
                rgb, shaded = fg.shade(S, ldir, rgba, g_cell, Tg)
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
    if n_surf:
        r["t"] = np.where(marched, prev.astype(F), r["t"])
        r["depth"] = r["depth"] | np.where(marched, sc.SIDES, 0).astype(np.int32)
    march.crossings, march.shaded = crossings, n_shaded
    march.shaded_ids = np.unique(np.concatenate(shaded_ids)) if shaded_ids else np.zeros(0, np.int64)
    if counts is not None:
        counts["refined"] = counts.get("refined", 0) + refined
        counts["crossings_refined"] = counts.get("crossings_refined", 0) + crossings_refined
    return r


def _walk(bricks, lo, hi, order, minv, cam, S, mode, plane, T, events, G, O, counts=None):
    """volume_mesh_shadow_checker._walk around the march above."""
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
        out = march(bricks[b], S, rays[here], minv, mode, T, events, G, O, counts)
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


def frame(bricks, lo, hi, minv, cam, S, mode=lc.SHADE_NONE, G=None, O=None, plane=None, bias=2):
    """gvt_hip_volume_frame_shadowed (G None, O None), _fog_shadowed (O None) or _mesh_shadowed with GVT_HIP_VOLUME_ALLOW_AMR over
    `bricks`, S (lights; surfaces or none) and the mode on every brick: the (H, W, 4) un-clamped framebuffer and the counters of
    volume_fog_shadow_checker.frame, plus "amr": {"refined", "crossings_refined": the camera rays'; "shadow_refined",
    "shadow_transitions": the shadow rays' (shadow_opacity's counts)}, plus details as volume_shadow_checker.frame's under "details"."""
    assert len(S.lpos) and 1 <= bias <= 64
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    T = None
    extra = {"shadow_rays": 0, "shadow_brick_visits": 0, "shadow_crossings": 0}
    amr = {"refined": 0, "crossings_refined": 0, "shadow_refined": 0, "shadow_transitions": 0}
    details = None
    if len(S):
        events = []
        _walk(bricks, lo, hi, order, minv, cam, S, mode, plane, None, events, None, O)  # (opacity never depends on colour: the samples are the same)
        ids = np.concatenate([e[0] for e in events]) if events else np.zeros(0, np.int64)
        ks = np.concatenate([e[1] for e in events]) if events else np.zeros(0, np.int64)
        wp = np.concatenate([e[2] for e in events]) if events else np.zeros((0, 3), F)
        ws, usable = sw.light_rays(S)
        A_s = np.zeros((len(ids), len(ws)), F)
        t_min = F(bias - 1) * bricks[0].dt
        sc_ = {}
        for j in np.nonzero(usable)[0]:
            A_s[:, j], v, c = shadow_opacity(bricks, lo, hi, order, minv, S, wp, np.broadcast_to(ws[j], wp.shape), t_min, sc_)
            extra["shadow_brick_visits"] += v
            extra["shadow_crossings"] += c
        extra["shadow_rays"] = len(ids) * int(usable.sum())
        amr["shadow_refined"], amr["shadow_transitions"] = sc_.get("refined", 0), sc_.get("transitions", 0)
        T = sw.Transmittance(sw._keys(ids, ks), (F(1) - A_s).astype(F))
        details = {"ids": ids, "k": ks, "A_s": A_s, "usable": usable}
    cnt = {}
    fb, counters = _walk(bricks, lo, hi, order, minv, cam, S, mode, plane, T, None, G, O, cnt)
    amr["refined"], amr["crossings_refined"] = cnt.get("refined", 0), cnt.get("crossings_refined", 0)
    counters.update(extra)
    counters["amr"] = amr
    counters["details"] = details
    return fb, counters
