"""numpy float32 restatement of the LIT VOLUME contract (include/gvt_hip.h, vol_accumulate_lit in gravit_amd/csrc/volume.hip), built on
tests/volume_checker.py, tests/volume_surface_checker.py and tests/volume_clip_checker.py: every sample the table gives opacity is
shaded by the gradient of the trilinear interpolant in its own cell, with the lights and ka / kd of the surfaces.  One march covers the
plain, the surface and the clipped march (a ray that carries CLIP ends at its t_max), each with shading on or off; with shading off it is
its parents' march bit for bit (tests/test_volume_shade_host.py).  Like its parents it interpolates every sample; every operation is one
IEEE float32 operation in the library's order.  march.shaded / frame.shaded: the samples shaded by the last call."""
import numpy as np

from gravit_amd.layouts import RAY_DTYPE
from oracle import orc
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_surface_checker as sc

F = vc.F
SHADE_NONE, SHADE_GRADIENT = 0, 1


def lights_only(lights, ka=0.4, kd=0.6):
    """What a volume without surfaces holds after set_lights."""
    return sc.Surfaces(lights=lights, ka=ka, kd=kd)


def gradient(B, v, fx, fy, fz):
    """The interpolant's gradient at the fractions, v = the cell's eight vertices in the order v000 v100 v010 v110 v001 v101 v011 v111."""
    v000, v100, v010, v110, v001, v101, v011, v111 = v
    lerp = vc.lerp
    with np.errstate(all="ignore"):
        return np.stack([
            lerp(lerp(v100 - v000, v110 - v010, fy), lerp(v101 - v001, v111 - v011, fy), fz) / B.sp[0],
            lerp(lerp(v010 - v000, v110 - v100, fx), lerp(v011 - v001, v111 - v101, fx), fz) / B.sp[1],
            lerp(lerp(v001 - v000, v101 - v100, fx), lerp(v011 - v010, v111 - v110, fx), fy) / B.sp[2]], axis=1).astype(F)


def shade(S, ldir, rgba, g):
    """The shaded sample's colour: rgba (n, 4) the look-up, g (n, 3) the gradient.  Returns (rgb (n, 3), shaded (n,) bool)."""
    with np.errstate(all="ignore"):
        shaded = rgba[:, 3] > 0
        ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F)
        ok = (ln > 0) & (ln < np.inf)
        nrm = (g / np.where(ok, ln, F(1))[:, None]).astype(F)
        tot = np.zeros((len(g), 3), F)
        for j in range(len(ldir)):
            ndl = np.abs((nrm[:, 0] * ldir[j, 0] + nrm[:, 1] * ldir[j, 1]) + nrm[:, 2] * ldir[j, 2]).astype(F)
            tot = (tot + S.lcol[j][None, :] * ndl[:, None]).astype(F)
        tot = np.where(ok[:, None], tot, F(0))
        lit = (rgba[:, :3] * (S.ka + S.kd * tot)).astype(F)
        return np.where(shaded[:, None], lit, rgba[:, :3]).astype(F), shaded


def march(B, S, rays, minv, mode=SHADE_GRADIENT):
    """gvt_hip_volume_trace on a RAY_DTYPE array (the marched copy).  S: a volume_surface_checker.Surfaces (its lights shade the samples
    too; None: nothing set).  Shading applies with mode GRADIENT and at least one light."""
    n_surf = 0 if S is None else len(S)
    lit = mode == SHADE_GRADIENT and S is not None and len(S.lpos) > 0
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
    ldir = S.light_dirs(minv) if S is not None else np.zeros((0, 3), F)
    n_iso = len(S.iso) if n_surf else 0
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
            g_cell = gradient(B, v8, fx, fy, fz) if lit or n_iso else None
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
                    Cj[sel], Aj[sel] = sc.composite(S, ldir, col, g, Cj[sel], Aj[sel])
                stop = (crossed != 0) & (Aj >= vc.OPAQUE_A)  # the surface ends the ray: the sample itself adds nothing
            rgba = sc.lookup(B, v)
            rgb = rgba[:, :3]
            if lit:
                rgb, shaded = shade(S, ldir, rgba, g_cell)
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
    if n_surf:
        r["t"] = np.where(marched, prev.astype(F), r["t"])
        r["depth"] = r["depth"] | np.where(marched, sc.SIDES, 0).astype(np.int32)
    march.crossings, march.shaded = crossings, n_shaded
    return r


def frame(bricks, lo, hi, minv, cam, S=None, mode=SHADE_GRADIENT, plane=None):
    """gvt_hip_volume_frame / _frame_clipped (plane: (H, W) depths, or None) with S and the mode on every brick: the (H, W, 4) un-clamped
    framebuffer and the marches; frame.shaded = the samples shaded by all of them."""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    fb = np.zeros((cam.width * cam.height, 4), F)
    queues = [[] for _ in bricks]
    flat = None if plane is None else np.ascontiguousarray(plane, F).reshape(-1)
    cc.shuffle(lo, hi, order, vc.camera_rays(cam), -1, queues, fb, flat)
    calls = shaded = 0
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
        rays = march(bricks[target], S, rays, minv, mode)
        shaded += march.shaded
        calls += 1
        cc.shuffle(lo, hi, order, rays, target, queues, fb)
    frame.shaded = shaded
    return fb.reshape(cam.height, cam.width, 4), calls
