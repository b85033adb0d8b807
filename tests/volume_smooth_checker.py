"""numpy float32 restatement of the SMOOTH GRADIENT contract (include/gvt_hip.h, vol_gradient_central in gravit_amd/csrc/volume.hip), built
on tests/volume_checker.py, tests/volume_surface_checker.py, tests/volume_clip_checker.py and tests/volume_shade_checker.py: with kind
CENTRAL a crossed isovalue and a lit sample are shaded by central differences at the cell's eight vertices, interpolated trilinearly;
with kind CELL the march is volume_shade_checker.march bit for bit (tests/test_volume_smooth_host.py).  A Brick here is the brick plus
the six face layers beyond it, given as such (a scenes.Brick that carries `ghosts`) or taken from the global grid.  The differences are
stated on GLOBAL vertex indices over a padded copy of the brick -- not the way the kernel finds its neighbours.  Every operation is one
IEEE float32 operation in the library's order."""
import numpy as np

from gravit_amd import scenes
from gravit_amd.layouts import RAY_DTYPE
from oracle import orc
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_shade_checker as lc
from tests import volume_surface_checker as sc

F = vc.F
SHADE_NONE, SHADE_GRADIENT = lc.SHADE_NONE, lc.SHADE_GRADIENT
CELL, CENTRAL = 0, 1


class Brick(vc.Brick):
    """volume_checker.Brick plus what gvt_hip_volume_set_ghosts holds.  grid (a scenes.VolumeData: the global grid the brick was cut
    from): the faces are taken from it; otherwise they are brick.ghosts (six arrays or None each; a whole VolumeData needs none)."""

    def __init__(self, brick, tf, sampling_rate=1.0, grid=None):
        super().__init__(brick, tf, sampling_rate)
        self.gn = np.asarray(getattr(brick, "global_counts", self.n), np.int64)
        if grid is not None:
            off = [int(v) for v in self.off]
            faces = scenes.brick_ghosts(grid.data, off, [o + int(n) - 1 for o, n in zip(off, self.n)])
        else:
            faces = getattr(brick, "ghosts", None) or [None] * 6
        self.set_ghosts(faces)

    def set_ghosts(self, faces):
        """pad[k + 1, j + 1, i + 1] = the vertex (i, j, k) relative to the brick, one layer beyond every face; NaN where nothing is known
        (a missing layer, the edges and the corners: the contract never reads them)."""
        nx, ny, nz = (int(v) for v in self.n)
        self.ghosts = [None if f is None else np.ascontiguousarray(f, F) for f in faces]
        self.pad = np.full((nz + 2, ny + 2, nx + 2), np.nan, F)
        self.pad[1:-1, 1:-1, 1:-1] = self.vox
        where = [np.s_[1:-1, 1:-1, 0], np.s_[1:-1, 1:-1, -1], np.s_[1:-1, 0, 1:-1], np.s_[1:-1, -1, 1:-1], np.s_[0, 1:-1, 1:-1], np.s_[-1, 1:-1, 1:-1]]
        for w, f in zip(where, self.ghosts):
            if f is not None:
                self.pad[w] = f

    def has_required_ghosts(self):
        """What gvt_hip_volume_set_gradient(CENTRAL) asks: a layer beyond every face that is not on the global boundary."""
        need = [self.off[0] > 0, self.off[0] + self.n[0] < self.gn[0], self.off[1] > 0, self.off[1] + self.n[1] < self.gn[1],
                self.off[2] > 0, self.off[2] + self.n[2] < self.gn[2]]
        return all(g is not None for g, n in zip(self.ghosts, need) if n)


def vertex_gradient(B, a, i, j, k):
    """Component a of the central difference at the vertices (i, j, k) relative to the brick (arrays): (v[ip] - v[im]) / (s * (float)(ip - im))
    on the axis' GLOBAL indices, im = max(g - 1, 0), ip = min(g + 1, N - 1)."""
    idx = [i, j, k]
    g = idx[a] + B.off[a]
    im, ip = np.maximum(g - 1, 0), np.minimum(g + 1, B.gn[a] - 1)
    lo, hi = list(idx), list(idx)
    lo[a], hi[a] = im - B.off[a], ip - B.off[a]
    with np.errstate(all="ignore"):
        vm = B.pad[lo[2] + 1, lo[1] + 1, lo[0] + 1]
        vp = B.pad[hi[2] + 1, hi[1] + 1, hi[0] + 1]
        return ((vp - vm) / (B.sp[a] * (ip - im).astype(F))).astype(F)


def central_gradient(B, c, fx, fy, fz):
    """(n, 3): per component the trilinear interpolation of the eight vertices' central differences, vol_gather's nesting (x, y, z)."""
    out = []
    lerp = vc.lerp
    with np.errstate(all="ignore"):
        for a in range(3):
            g = {(dx, dy, dz): vertex_gradient(B, a, c[:, 0] + dx, c[:, 1] + dy, c[:, 2] + dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
            c00, c10 = lerp(g[0, 0, 0], g[1, 0, 0], fx), lerp(g[0, 1, 0], g[1, 1, 0], fx)
            c01, c11 = lerp(g[0, 0, 1], g[1, 0, 1], fx), lerp(g[0, 1, 1], g[1, 1, 1], fx)
            out.append(lerp(lerp(c00, c10, fy), lerp(c01, c11, fy), fz))
    return np.stack(out, axis=1).astype(F)


def march(B, S, rays, minv, mode=SHADE_GRADIENT, kind=CELL):
    """gvt_hip_volume_trace on a RAY_DTYPE array (the marched copy), as volume_shade_checker.march; kind: the gradient that shades a
    crossed isovalue and a lit sample.  B: a Brick of this module for CENTRAL (any volume_checker.Brick for CELL)."""
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
            g_cell = None
            if lit or n_iso:
                g_cell = central_gradient(B, c, fx, fy, fz) if kind == CENTRAL else lc.gradient(B, v8, fx, fy, fz)
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
    if n_surf:
        r["t"] = np.where(marched, prev.astype(F), r["t"])
        r["depth"] = r["depth"] | np.where(marched, sc.SIDES, 0).astype(np.int32)
    march.crossings, march.shaded = crossings, n_shaded
    return r


def frame(bricks, lo, hi, minv, cam, S=None, mode=SHADE_GRADIENT, plane=None, kind=CELL):
    """gvt_hip_volume_frame / _frame_clipped (plane: (H, W) depths, or None) with S and the mode on every brick: the (H, W, 4) un-clamped
    framebuffer and the marches; frame.shaded / frame.crossings = the samples shaded and the surfaces composited by all of them."""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    fb = np.zeros((cam.width * cam.height, 4), F)
    queues = [[] for _ in bricks]
    flat = None if plane is None else np.ascontiguousarray(plane, F).reshape(-1)
    cc.shuffle(lo, hi, order, vc.camera_rays(cam), -1, queues, fb, flat)
    calls = shaded = crossings = 0
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
        rays = march(bricks[target], S, rays, minv, mode, kind)
        shaded += march.shaded
        crossings += march.crossings
        calls += 1
        cc.shuffle(lo, hi, order, rays, target, queues, fb)
    frame.shaded, frame.crossings = shaded, crossings
    return fb.reshape(cam.height, cam.width, 4), calls
