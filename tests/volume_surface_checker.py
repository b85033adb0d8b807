"""numpy float32 restatement of the volume SURFACE contract (include/gvt_hip.h, k_volume_march_surf in gravit_amd/csrc/volume.hip), built
on tests/volume_checker.py: isovalues and slice planes detected between consecutive lattice samples, shaded and composited before the
sample's own contribution, and the side mask a ray carries from brick to brick (its t field and the RAY_SIDES bit of depth).  Like its
parent it interpolates every sample; every operation is one IEEE float32 operation in the library's order."""
import numpy as np

from gravit_amd.layouts import RAY_DTYPE
from oracle import orc
from tests import volume_checker as vc

F = vc.F
SIDES = 0x20
MAX_SURFACES, MAX_LIGHTS = 16, 8


class Surfaces:
    """What gvt_hip_volume_set_surfaces + _set_lights hold: isovalues, planes (nx, ny, nz, d), one opacity; lights = (position, colour)
    pairs in world space."""

    def __init__(self, isovalues=(), slices=(), opacity=1.0, lights=(), ka=0.4, kd=0.6):
        self.iso = np.asarray(isovalues, F).reshape(-1)
        self.planes = np.asarray(slices, F).reshape(-1, 4) if len(slices) else np.zeros((0, 4), F)
        assert len(self.iso) + len(self.planes) <= MAX_SURFACES and len(lights) <= MAX_LIGHTS
        self.opacity = F(opacity)
        self.lpos = np.asarray([l[0] for l in lights], F).reshape(-1, 3)
        self.lcol = np.asarray([l[1] for l in lights], F).reshape(-1, 3)
        self.ka, self.kd = F(ka), F(kd)

    def __len__(self):
        return len(self.iso) + len(self.planes)

    def light_dirs(self, minv):
        """-position as a vector through minv, normalised (length 0 or not finite: 0) -- the host's computation at every march."""
        if not len(self.lpos):
            return np.zeros((0, 3), F)
        with np.errstate(all="ignore"):
            l = vc.xfm_vector(minv, (-self.lpos).astype(F))
            ln = np.sqrt((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) + l[:, 2] * l[:, 2]).astype(F)
            ok = (ln > 0) & np.isfinite(ln)
            return np.where(ok[:, None], l / np.where(ok, ln, F(1))[:, None], F(0)).astype(F)


def lookup(B, v):
    """The sample's table look-up at values v: (n, 4)."""
    with np.errstate(all="ignore"):
        pos = np.fmin(np.fmax((v - B.vlo) / B.vspan, F(0)), F(1)) * F(255)
        i0 = np.minimum(np.nan_to_num(pos).astype(np.int64), 254)
        w = (pos - i0.astype(F)).astype(F)
        return vc.lerp(B.tf[i0], B.tf[i0 + 1], w[:, None]).astype(F)


def composite(S, ldir, c, g, C, A):
    """One crossed surface per row: base colour c (n, 3), unnormalised normal g (n, 3); returns the new (C, A)."""
    rgb = c
    with np.errstate(all="ignore"):
        if len(ldir):
            ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F)
            ok = ln > 0
            nrm = (g / np.where(ok, ln, F(1))[:, None]).astype(F)
            tot = np.zeros_like(c)
            for j in range(len(ldir)):
                ndl = np.abs((nrm[:, 0] * ldir[j, 0] + nrm[:, 1] * ldir[j, 1]) + nrm[:, 2] * ldir[j, 2]).astype(F)
                tot = (tot + S.lcol[j][None, :] * ndl[:, None]).astype(F)
            tot = np.where(ok[:, None], tot, F(0))
            rgb = (c * (S.ka + S.kd * tot)).astype(F)
        f = ((F(1) - A) * S.opacity).astype(F)
        return (C + f[:, None] * rgb).astype(F), (A + f).astype(F)


def march(B, S, rays, minv):
    """k_volume_march_surf on a RAY_DTYPE array (the marched copy).  S = None or no surfaces: the plain march of the parent checker."""
    if S is None or not len(S):
        return vc.march(B, rays, minv)
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
    k_last = np.full(n, -1, np.int64)
    seen = np.zeros(n, bool)
    carried = (r["depth"] & SIDES) != 0
    with np.errstate(all="ignore"):
        prev = np.where(carried, np.nan_to_num(r["t"]).astype(np.int64) & 0xFFFF, -1)
    k_carry = np.where(carried, kp, -1)
    ldir = S.light_dirs(minv)
    n_iso = len(S.iso)
    active = k <= k_hi
    nx, ny = int(B.n[0]), int(B.n[1])
    flat = B.vox.reshape(-1)
    crossings = 0
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
        prev[j[first & (k[j] != k_carry[j])]] = -1  # the carried sides belong to the sample right before this one, or to none
        seen[j] = True
        k_last[j] = k[j]
        t = k[j].astype(F) * B.dt
        p = (o[j] + d[j] * t[:, None]).astype(F)
        base = c[:, 0] + nx * c[:, 1] + nx * ny * c[:, 2]
        sy, sz = nx, nx * ny
        v000, v100, v010, v110 = flat[base], flat[base + 1], flat[base + sy], flat[base + sy + 1]
        v001, v101, v011, v111 = flat[base + sz], flat[base + sz + 1], flat[base + sz + sy], flat[base + sz + sy + 1]
        fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
        with np.errstate(all="ignore"):
            c00, c10 = vc.lerp(v000, v100, fx), vc.lerp(v010, v110, fx)
            c01, c11 = vc.lerp(v001, v101, fx), vc.lerp(v011, v111, fx)
            c0, c1 = vc.lerp(c00, c10, fy), vc.lerp(c01, c11, fy)
            v = vc.lerp(c0, c1, fz)
            sides = np.zeros(len(j), np.int64)
            for i in range(n_iso):
                sides |= (v >= S.iso[i]).astype(np.int64) << i
            for i, P in enumerate(S.planes):
                sides |= (((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) >= P[3]).astype(np.int64) << (n_iso + i)
            crossed = np.where(prev[j] < 0, 0, sides ^ prev[j])
            prev[j] = sides
            Cj, Aj = C[j], A[j]
            if crossed.any():
                g_iso = None
                for i in range(len(S)):
                    sel = ((crossed >> i) & 1).astype(bool) & (Aj < vc.OPAQUE_A)
                    if not sel.any():
                        continue
                    crossings += int(sel.sum())
                    if i < n_iso:
                        if g_iso is None:
                            g_iso = np.stack([
                                vc.lerp(vc.lerp(v100 - v000, v110 - v010, fy), vc.lerp(v101 - v001, v111 - v011, fy), fz) / B.sp[0],
                                vc.lerp(vc.lerp(v010 - v000, v110 - v100, fx), vc.lerp(v011 - v001, v111 - v101, fx), fz) / B.sp[1],
                                vc.lerp(vc.lerp(v001 - v000, v101 - v100, fx), vc.lerp(v011 - v010, v111 - v110, fx), fy) / B.sp[2]],
                                axis=1).astype(F)
                        col = lookup(B, np.full(int(sel.sum()), S.iso[i], F))[:, :3]
                        g = g_iso[sel]
                    else:
                        col = lookup(B, v[sel])[:, :3]
                        g = np.broadcast_to(S.planes[i - n_iso][:3], (int(sel.sum()), 3)).astype(F)
                    Cj[sel], Aj[sel] = composite(S, ldir, col, g, Cj[sel], Aj[sel])
            stop = (crossed != 0) & (Aj >= vc.OPAQUE_A)  # the surface ends the ray: the sample itself adds nothing
            rgba = lookup(B, v)
            fr = ((F(1) - Aj) * rgba[:, 3]).astype(F)
            Cn = (Cj + fr[:, None] * rgba[:, :3]).astype(F)
            An = (Aj + fr).astype(F)
        C[j] = np.where(stop[:, None], Cj, Cn)
        A[j] = np.where(stop, Aj, An)
        k[j] += 1
        active[j[A[j] >= vc.OPAQUE_A]] = False
    marched = k_last >= 0
    r["t_min"] = np.where(marched, k_last.astype(F) * B.dt, r["t_min"])
    r["t"] = np.where(marched, prev.astype(F), r["t"])
    r["color"] = C
    r["w"] = A
    r["depth"] = r["depth"] | np.where(A >= vc.OPAQUE_A, vc.OPAQUE, vc.BOUNDARY).astype(np.int32) | np.where(marched, SIDES, 0).astype(np.int32)
    march.crossings = crossings
    return r


def frame(bricks, lo, hi, minv, cam, S=None, final=None):
    """gvt_hip_volume_frame with surfaces on every brick: the parent's loop around this module's march.  final (a list): gets every ray
    as it is deposited or dropped after a march (its last state)."""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    fb = np.zeros((cam.width * cam.height, 4), F)
    queues = [[] for _ in bricks]
    vc.shuffle(lo, hi, order, vc.camera_rays(cam), -1, queues, fb)
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
        rays = march(bricks[target], S, rays, minv)
        calls += 1
        before = [sum(len(a) for a in q) for q in queues]
        vc.shuffle(lo, hi, order, rays, target, queues, fb)
        if final is not None:
            moved = sum(sum(len(a) for a in q) for q in queues) - sum(before)
            # the rays that went nowhere ended here: OPAQUE, or BOUNDARY with no next brick
            nxt = np.full(len(rays), -1, np.int64)
            bnd = ((rays["depth"] & vc.OPAQUE) == 0) & ((rays["depth"] & vc.BOUNDARY) != 0)
            if bnd.any():
                nxt[bnd] = vc.next_brick(lo, hi, order, rays[bnd], target)
            assert (nxt >= 0).sum() == moved
            final.append(rays[nxt < 0])
    return fb.reshape(cam.height, cam.width, 4), calls
