"""numpy float32 restatement of "AMR volumes: surfaces and lit fog" (include/gvt_hip.h, GVT_HIP_VOLUME_AMR_SHADED; k_volume_march_amr_surf /
_lit / _surf_lit in gravit_amd/csrc/volume_amr.inc): tests/volume_amr_checker.py's march loop with tests/volume_surface_checker.py's
crossing / composite step and tests/volume_shade_checker.py's shading.  The value, the eight corners and the fractions of a sample are
those of the FINAL grid's cell after the descent (ac.descend), and the gradient divides by the final grid's spacing s_a = spacing.a /
(float)R, R the product of the ratios down to that grid.  Plane sides read the lattice point.  Like its parents it interpolates every
sample (no skipping), honours the clip on rays that carry it, and every operation is one IEEE float32 operation in the library's order."""
import numpy as np

from gravit_amd.layouts import RAY_DTYPE
from oracle import orc
from tests import volume_amr_checker as ac
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_shade_checker as shc
from tests import volume_surface_checker as sc

F = vc.F
SHADE_NONE, SHADE_GRADIENT = shc.SHADE_NONE, shc.SHADE_GRADIENT
COUNT_KEYS = ("marched", "refined", "crossings", "crossings_refined", "crossings_grid_change", "plane_crossings_refined", "shaded", "shaded_refined",
              "carried_refined")


def levels(B):
    """Per subgrid: its level (1 for a child of the brick's grid) and R, the product of the ratios down to it."""
    lev, rt = [], []
    for parent, ratio, _, _, _ in B.sub:
        lev.append(1 if parent < 0 else lev[parent] + 1)
        rt.append(ratio if parent < 0 else rt[parent] * ratio)
    return np.asarray(lev, np.int64), np.asarray(rt, np.int64)


def corners(B, grid, ci):
    """The eight vertices of cell ci of each sample's final grid, in the order v000 v100 v010 v110 v001 v101 v011 v111."""
    out = [np.zeros(len(grid), F) for _ in range(8)]
    for g in np.unique(grid):
        m = grid == g
        data = B.vox if g < 0 else B.sub[g][4]
        nz, ny, nx = data.shape
        flat = data.reshape(-1)
        c = ci[m]
        base = c[:, 0] + nx * c[:, 1] + nx * ny * c[:, 2]
        sy, sz = nx, nx * ny
        for q, off in enumerate((0, 1, sy, sy + 1, sz, sz + 1, sz + sy, sz + sy + 1)):
            out[q][m] = flat[base + off]
    return tuple(out)


def gradient(B, v8, f, R):
    """The interpolant's gradient in the final cell: the header's lerp nest of corner differences, divided by s_a = spacing.a / (float)R."""
    v000, v100, v010, v110, v001, v101, v011, v111 = v8
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    lerp = vc.lerp
    with np.errstate(all="ignore"):
        Rf = R.astype(F)
        s = [(B.sp[a] / Rf).astype(F) for a in range(3)]
        return np.stack([
            lerp(lerp(v100 - v000, v110 - v010, fy), lerp(v101 - v001, v111 - v011, fy), fz) / s[0],
            lerp(lerp(v010 - v000, v110 - v100, fx), lerp(v011 - v001, v111 - v101, fx), fz) / s[1],
            lerp(lerp(v001 - v000, v101 - v100, fx), lerp(v011 - v010, v111 - v110, fx), fy) / s[2]], axis=1).astype(F)


def march(B, S, rays, minv, mode=SHADE_GRADIENT, counts=None):
    """gvt_hip_volume_trace of a flagged AMR brick on a RAY_DTYPE array (the marched copy).  B: an ac.AmrBrick; S: a
    volume_surface_checker.Surfaces (None: nothing set); shading applies with mode GRADIENT and at least one light.  counts (a dict) is
    added to: COUNT_KEYS and "crossings_level" (a dict level -> crossings detected at samples whose final grid has that level).  A
    crossing "at a grid change": the final grid of the sample differs from the one of the previous sample of this visit.
    "carried_refined": rays whose first owned sample took the sides carried in t and lies in a subgrid."""
    n_surf = 0 if S is None else len(S)
    lit = mode == SHADE_GRADIENT and S is not None and len(S.lpos) > 0
    lev, rt = levels(B)
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
    prev_grid = np.full(n, -2, np.int64)  # the final grid of the previous sample of this visit (-2: none)
    ldir = S.light_dirs(minv) if S is not None else np.zeros((0, 3), F)
    n_iso = len(S.iso) if n_surf else 0
    active = k <= k_hi
    cnt = dict.fromkeys(COUNT_KEYS, 0)
    per_level = {}
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
        first = ~seen[j]
        prev[j[first & (k[j] != k_carry[j])]] = -1
        seen[j] = True
        k_last[j] = k[j]
        t = k[j].astype(F) * B.dt
        p = (o[j] + d[j] * t[:, None]).astype(F)
        grid, ci, ff = ac.descend(B, c[own], f[own])
        fine = grid >= 0
        glev = np.where(fine, lev[np.maximum(grid, 0)] if len(lev) else 0, 0)
        R = np.where(fine, rt[np.maximum(grid, 0)] if len(rt) else 1, 1)
        cnt["marched"] += len(j)
        cnt["refined"] += int(fine.sum())
        cnt["carried_refined"] += int((first & (k[j] == k_carry[j]) & (prev[j] >= 0) & fine).sum()) if n_surf else 0
        v8 = corners(B, grid, ci)
        v000, v100, v010, v110, v001, v101, v011, v111 = v8
        fx, fy, fz = ff[:, 0], ff[:, 1], ff[:, 2]
        with np.errstate(all="ignore"):
            c00, c10 = vc.lerp(v000, v100, fx), vc.lerp(v010, v110, fx)
            c01, c11 = vc.lerp(v001, v101, fx), vc.lerp(v011, v111, fx)
            c0, c1 = vc.lerp(c00, c10, fy), vc.lerp(c01, c11, fy)
            v = vc.lerp(c0, c1, fz)
            g_cell = gradient(B, v8, ff, R) if lit or n_iso else None
            Cj, Aj = C[j], A[j]
            stop = np.zeros(len(j), bool)
            if n_surf:
                sides = np.zeros(len(j), np.int64)
                for i in range(n_iso):
                    sides |= (v >= S.iso[i]).astype(np.int64) << i
                for i, P in enumerate(S.planes):
                    sides |= (((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) >= P[3]).astype(np.int64) << (n_iso + i)
                crossed = np.where(prev[j] < 0, 0, sides ^ prev[j])
                prev[j] = sides
                changed = (prev_grid[j] != -2) & (prev_grid[j] != grid)
                for i in range(n_surf):
                    sel = ((crossed >> i) & 1).astype(bool) & (Aj < vc.OPAQUE_A)
                    if not sel.any():
                        continue
                    cnt["crossings"] += int(sel.sum())
                    cnt["crossings_refined"] += int((sel & fine).sum())
                    cnt["crossings_grid_change"] += int((sel & changed).sum())
                    for l in np.unique(glev[sel]):
                        per_level[int(l)] = per_level.get(int(l), 0) + int((sel & (glev == l)).sum())
                    if i < n_iso:
                        col = sc.lookup(B, np.full(int(sel.sum()), S.iso[i], F))[:, :3]
                        g = g_cell[sel]
                    else:
                        cnt["plane_crossings_refined"] += int((sel & fine).sum())
                        col = sc.lookup(B, v[sel])[:, :3]
                        g = np.broadcast_to(S.planes[i - n_iso][:3], (int(sel.sum()), 3)).astype(F)
                    Cj[sel], Aj[sel] = sc.composite(S, ldir, col, g, Cj[sel], Aj[sel])
                stop = (crossed != 0) & (Aj >= vc.OPAQUE_A)  # the surface ends the ray: the sample itself adds nothing
            prev_grid[j] = grid
            rgba = sc.lookup(B, v)
            rgb = rgba[:, :3]
            if lit:
                rgb, shaded = shc.shade(S, ldir, rgba, g_cell)
                cnt["shaded"] += int((shaded & ~stop).sum())
                cnt["shaded_refined"] += int((shaded & ~stop & fine).sum())
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
    if counts is not None:
        for key in COUNT_KEYS:
            counts[key] = counts.get(key, 0) + cnt[key]
        lv = counts.setdefault("crossings_level", {})
        for l, c_ in per_level.items():
            lv[l] = lv.get(l, 0) + c_
    return r


def frame(bricks, lo, hi, minv, cam, S=None, mode=SHADE_GRADIENT, plane=None, counts=None, rounds=None):
    """gvt_hip_volume_frame / _frame_clipped (plane: (H, W) depths, or None) over flagged AMR bricks with S and the mode on every brick:
    ac.frame's loop with this module's march.  Returns the (H, W, 4) un-clamped framebuffer and the marches; counts as march's, summed;
    rounds (a list): gets each round's (brick, rays)."""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    fb = np.zeros((cam.width * cam.height, 4), F)
    queues = [[] for _ in bricks]
    flat = None if plane is None else np.ascontiguousarray(plane, F).reshape(-1)
    cc.shuffle(lo, hi, order, vc.camera_rays(cam), -1, queues, fb, flat)
    calls = 0
    while True:
        sizes = [sum(len(a) for a in q) for q in queues]
        target, best = -1, 0
        for i, s in enumerate(sizes):
            if s > best:
                best, target = s, i
        if target < 0:
            break
        rays = np.concatenate(queues[target]) if queues[target] else np.zeros(0, RAY_DTYPE)
        queues[target] = []
        if rounds is not None:
            rounds.append((target, len(rays)))
        rays = march(bricks[target], S, rays, minv, mode, counts)
        calls += 1
        cc.shuffle(lo, hi, order, rays, target, queues, fb)
    return fb.reshape(cam.height, cam.width, 4), calls
