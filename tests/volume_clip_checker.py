"""numpy float32 restatement of "geometry inside a volume" (include/gvt_hip.h): the plain march clipped at a ray's t_max
(GVT_HIP_RAY_CLIP), gvt_hip_shuffle_volume's rule with the tn < t_max cut, the clipped frame and the composite.  Built on
tests/volume_checker.py's helpers; the march loop is restated because its k_hi is internal to vc.march (test_volume_clip_host.py ties
the two together: with no ray flagged they agree bit for bit)."""
import numpy as np

from gravit_amd.layouts import RAY_DTYPE
from oracle import orc
from tests import volume_checker as vc

F = np.float32
CLIP = 0x40
INF = F(np.inf)


def last_before(t_max, dt):
    """vol_last_before: the largest k >= 0 with (float)k * dt < t_max; -1: none (t_max <= 0, NaN); 2^30: no cut (+Inf, or too far)."""
    t = np.asarray(t_max, F)
    k = np.full(len(t), -1, np.int64)
    with np.errstate(all="ignore"):
        pos = t > 0
        q = np.floor(t / dt)
        nocut = pos & ~(q < vc.K_MAX)
        use = pos & ~nocut
        k[use] = q[use].astype(np.int64)
        while True:
            up = use & ((k + 1).astype(F) * dt < t)
            if not up.any():
                break
            k[up] += 1
        while True:
            dn = use & (k >= 0) & ~(k.astype(F) * dt < t)
            if not dn.any():
                break
            k[dn] -= 1
    k[nocut] = int(vc.K_MAX)
    return k


def march(B, rays, minv):
    """vc.march with the clip: a ray that carries CLIP walks k_hi = min(k_hi, last_before(t_max)); everything else as it was."""
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
    flagged = (r["depth"] & CLIP) != 0
    k_hi = np.where(ok & flagged, np.minimum(k_hi, last_before(r["t_max"], B.dt)), k_hi)  # the clip, last
    k_last = np.full(n, -1, np.int64)
    seen = np.zeros(n, bool)
    active = k <= k_hi
    nx, ny = int(B.n[0]), int(B.n[1])
    flat = B.vox.reshape(-1)
    lerp = vc.lerp
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
        seen[j] = True
        k_last[j] = k[j]
        base = c[:, 0] + nx * c[:, 1] + nx * ny * c[:, 2]
        sy, sz = nx, nx * ny
        v000, v100, v010, v110 = flat[base], flat[base + 1], flat[base + sy], flat[base + sy + 1]
        v001, v101, v011, v111 = flat[base + sz], flat[base + sz + 1], flat[base + sz + sy], flat[base + sz + sy + 1]
        c00, c10 = lerp(v000, v100, f[:, 0]), lerp(v010, v110, f[:, 0])
        c01, c11 = lerp(v001, v101, f[:, 0]), lerp(v011, v111, f[:, 0])
        c0, c1 = lerp(c00, c10, f[:, 1]), lerp(c01, c11, f[:, 1])
        v = lerp(c0, c1, f[:, 2])
        pos = np.fmin(np.fmax((v - B.vlo) / B.vspan, F(0)), F(1)) * F(255)
        i0 = np.minimum(pos.astype(np.int64), 254)
        w = (pos - i0.astype(F)).astype(F)
        e0, e1 = B.tf[i0], B.tf[i0 + 1]
        rgba = lerp(e0, e1, w[:, None]).astype(F)
        fr = ((F(1) - A[j]) * rgba[:, 3]).astype(F)
        C[j] = C[j] + fr[:, None] * rgba[:, :3]
        A[j] = A[j] + fr
        k[j] += 1
        active[j[A[j] >= vc.OPAQUE_A]] = False
    r["t_min"] = np.where(k_last >= 0, k_last.astype(F) * B.dt, r["t_min"])
    r["color"] = C
    r["w"] = A
    r["depth"] = r["depth"] | np.where(A >= vc.OPAQUE_A, vc.OPAQUE, vc.BOUNDARY).astype(np.int32)
    return r


def next_brick(lo, hi, order, rays, frm, clip=None, t_clip=None):
    """vol_next with the cut: for a clipped ray a box is a candidate only if its entry distance tn < t_clip.  clip / t_clip: per ray, by
    default the ray's own flag and t_max."""
    o, d = rays["origin"].astype(F), rays["direction"].astype(F)
    n = len(rays)
    clip = ((rays["depth"] & CLIP) != 0) if clip is None else clip
    t_clip = rays["t_max"].astype(F) if t_clip is None else t_clip
    p = rays["t_min"].astype(F).copy()
    if frm >= 0:
        p = vc.slab(lo[frm], hi[frm], o, d)[1]
    nxt = np.full(n, -1, np.int64)
    best = np.full(n, np.inf, F)
    with np.errstate(all="ignore"):
        for inst in order:
            if inst == frm:
                continue
            tn, tf = vc.slab(lo[inst], hi[inst], o, d)
            take = (tn <= tf) & (tf > p) & (~clip | (tn < t_clip)) & ((nxt < 0) | (tn < best))
            nxt[take] = inst
            best[take] = tn[take]
    return nxt


def shuffle(lo, hi, order, rays, frm, queues, fb, plane=None):
    """gvt_hip_shuffle_volume with the cut.  plane (frm < 0, the clipped frame; W*H floats): a camera ray is classified with, and
    enters its queue with, t_max = plane[id] and depth = CLIP where that is below +Inf, else 0."""
    depth = rays["depth"]
    if frm < 0:
        if plane is not None:
            t = plane[rays["id"].astype(np.int64)].astype(F)
            with np.errstate(all="ignore"):
                cut = t < INF
            nxt = next_brick(lo, hi, order, rays, -1, cut, t)
        else:
            nxt = next_brick(lo, hi, order, rays, -1)
        deposit = np.zeros(len(rays), bool)
    else:
        nxt = np.full(len(rays), -1, np.int64)
        bnd = ((depth & vc.OPAQUE) == 0) & ((depth & vc.BOUNDARY) != 0)
        if bnd.any():
            nxt[bnd] = next_brick(lo, hi, order, rays[bnd], frm)
        deposit = ((depth & vc.OPAQUE) != 0) | (bnd & (nxt < 0))
    dep = rays[deposit]
    ids = dep["id"].astype(np.int64)
    okid = (ids >= 0) & (ids < len(fb))
    np.add.at(fb, (ids[okid], slice(0, 3)), dep["color"][okid])
    np.add.at(fb, (ids[okid], 3), dep["w"][okid])
    for i in range(len(queues)):
        pick = nxt == i
        sel = rays[pick].copy()
        if not len(sel):
            continue
        sel["depth"] &= ~vc.BOUNDARY
        if frm < 0:
            sel["color"] = 0
            sel["w"] = 0
            sel["depth"] = 0
            if plane is not None:
                sel["t_max"] = t[pick]
                sel["depth"] = np.where(cut[pick], CLIP, 0)
        queues[i].append(sel)


def frame(bricks, lo, hi, minv, cam, plane=None):
    """gvt_hip_volume_frame_clipped: the (H, W, 4) un-clamped framebuffer and the marches.  plane: (H, W) floats, or None (the plain frame)."""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    fb = np.zeros((cam.width * cam.height, 4), F)
    queues = [[] for _ in bricks]
    flat = None if plane is None else np.ascontiguousarray(plane, F).reshape(-1)
    shuffle(lo, hi, order, vc.camera_rays(cam), -1, queues, fb, flat)
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
        rays = march(bricks[target], rays, minv)
        calls += 1
        shuffle(lo, hi, order, rays, target, queues, fb)
    return fb.reshape(cam.height, cam.width, 4), calls


def composite(front, back, depth=None):
    """gvt_hip_fb_composite_over: front over back, (H, W, 4) each; coverage from depth (H, W) or, without one, from back's alpha."""
    front, back = np.asarray(front, F), np.asarray(back, F)
    out = front.copy()
    k = (F(1) - front[..., 3]).astype(F)
    with np.errstate(all="ignore"):
        cov = np.fmin(back[..., 3], F(1)) if depth is None else np.where(np.asarray(depth, F) < INF, F(1), F(0)).astype(F)
        out[..., :3] = front[..., :3] + k[..., None] * np.fmin(back[..., :3], F(1))
        out[..., 3] = front[..., 3] + k * cov
    return out


def depth_of_plane(cam, normal, offset, keep):
    """A synthetic depth plane: t of every camera ray at the plane normal . p = offset (+Inf where it is not in front of the eye),
    computed in double and rounded once, and +Inf wherever `keep` (H, W bool) is false."""
    rays = vc.camera_rays(cam)
    o, d = rays["origin"].astype(np.float64), rays["direction"].astype(np.float64)
    nrm = np.asarray(normal, np.float64)
    with np.errstate(all="ignore"):
        t = (offset - o @ nrm) / (d @ nrm)
    t = np.where(np.isfinite(t) & (t > 0), t, np.inf)
    out = np.full(cam.width * cam.height, np.inf, F)
    out[rays["id"].astype(np.int64)] = t.astype(F)
    out = out.reshape(cam.height, cam.width)
    return np.where(keep, out, INF).astype(F)
