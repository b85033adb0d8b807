"""Shared builders of the volume march's edge cases (tests/test_volume_edges_host.py proves on the CPU that they are not vacuous,
tests/test_gpu_volume_edges.py runs them on the device): small non-cubic grids on a power-of-two geometry, block-wise plateaus next to
single-entry opacity spikes, non-finite and huge samples, narrow value ranges far from zero, values outside the table, thin and offset
bricks, and a ray list with the origins, directions, t_min and incoming opacities the friendly tests never give.  No GPU here."""
import numpy as np

from gravit_amd import scenes
from gravit_amd.adapter import TransferFunction
from gravit_amd.layouts import RAY_DTYPE
from tests import volume_checker as vc
from tests.test_gpu_volume import make_rays

F = np.float32
COUNTS = (19, 10, 27)                       # x y z vertices: 3 x 2 x 4 macro cells with tails of 2, 1 and 2 cells
SPACING = (1.0 / 16, 1.0 / 32, 1.0 / 8)     # powers of two: lattice points can land exactly on vertices and faces
ORIGIN = (-0.5, 0.25, -1.0)
GRAY = np.array([[0, 0.1, 0.2, 0.9], [0.5, 0.9, 0.8, 0.1], [1, 0.3, 1.0, 0.5]], F)
RATES = (0.11, 0.37, 1.0, 4.3)


def volume(data, spacing=SPACING, origin=ORIGIN):
    return scenes.VolumeData(np.ascontiguousarray(data, F), np.array(origin, F), np.array(spacing, F))


def block_of(counts=COUNTS):
    """Per vertex (z, y, x) its macro cell per axis: vertex 8b belongs to block b (and is the boundary vertex of block b - 1)."""
    nb = [(c - 1 + 7) // 8 for c in counts]
    ax = [np.minimum(np.arange(c) // 8, n - 1) for c, n in zip(counts, nb)]
    bz, by, bx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return bx, by, bz, nb


# ---- plateaus: block b = (bx, by, bz) holds the table entry E(b) (or E + 0.5) on all vertices it does not share with a block below it
def plateau_entry(bx, by, bz):
    return 10 + 6 * bx + 20 * by + 45 * bz


def plateaus(half=False):
    bx, by, bz, _ = block_of()
    e = plateau_entry(bx, by, bz).astype(np.float64) + (0.5 if half else 0.0)
    return volume((e / 255.0).astype(F))


def spike(e, peak=1.0, value_range=(0.0, 1.0)):
    """Opacity `peak` at table entry e only: the rows hit the resampling positions exactly, so entries e - 1 and e + 1 are exactly 0."""
    rows = [[0.0, 0.0]] if e > 1 else []
    rows += [[(e - 1) / 255.0, 0.0], [e / 255.0, peak], [(e + 1) / 255.0, 0.0]]
    if e < 254:
        rows.append([1.0, 0.0])
    return TransferFunction(GRAY, np.array(rows, F), value_range)


PLATEAU_BLOCK = plateau_entry(1, 1, 1)  # 81: a block with ramps towards its +x, +y and +z neighbours
PLATEAU_TAIL = plateau_entry(2, 1, 3)   # 177: the tail corner block, constant on every vertex
# spikes at distances 0, 1, 2 and 3 entries from those block values, either side (distance 3 above the tail block: every block is empty)
PLATEAU_SPIKES = (78, 79, 80, 81, 82, 84, 174, 176, 177, 178, 179, 180)


def broad():
    """Opacity everywhere: no block is empty."""
    return TransferFunction(GRAY, np.array([[0, 0.05], [0.4, 0.3], [1, 0.1]], F), (0.0, 1.0))


def faint():
    """Little opacity everywhere: most rays cross several bricks before they finish."""
    return TransferFunction(GRAY, np.array([[0, 0.0], [0.4, 0.04], [1, 0.01]], F), (0.0, 1.0))


# ---- nonfinite: 0.5 with a small ramp at the far x end, and a handful of vertices that are not numbers
NONFINITE_VERTS = ((4, 3, 4), (5, 3, 4), (8, 4, 12), (16, 8, 16), (0, 5, 20), (18, 2, 9), (10, 9, 26), (12, 0, 3))  # x y z: block interior (two
# neighbours), a block face, a block corner, the brick's outer faces


def nonfinite(kind):
    """kind: pinf, ninf, nan or mixed."""
    nx, ny, nz = COUNTS
    d = np.full((nz, ny, nx), 0.5, F)
    d[:, :, 16:] += (np.arange(nx - 16, dtype=F) * F(0.01))[None, None, :]
    vals = {"pinf": [np.inf], "ninf": [-np.inf], "nan": [np.nan], "mixed": [np.inf, -np.inf, np.nan]}[kind]
    for i, (x, y, z) in enumerate(NONFINITE_VERTS):
        d[z, y, x] = vals[i % len(vals)]
    return volume(d)


def nonfinite_table(where):
    """Opaque only at the bottom, only at the top, or only in the middle around 0.5."""
    omap = {"bottom": [[0, 1], [0.02, 0], [1, 0]], "top": [[0, 0], [0.98, 0], [1, 1]],
            "middle": [[0, 0], [0.45, 0], [0.5, 0.3], [0.55, 0], [1, 0]]}[where]
    return TransferFunction(GRAY, np.array(omap, F), (0.0, 1.0))


# ---- far_narrow: 1000 + 0.005 * noise.  One float32 step at 1000 is three table entries wide
def far_narrow(seed=4):
    """noise = 0.3 in the macro cells bz 0 and 1, 0.7 in bz 2 and 3, +-0.03 of jitter: the blocks bz = 0, 2 and 3 lie strictly between
    the spikes of far_narrow_table(), the blocks bz = 1 ramp through all of them."""
    bx, by, bz, _ = block_of()
    rng = np.random.default_rng(seed)
    noise = np.where(bz < 2, 0.3, 0.7) + 0.03 * (2 * rng.random(bz.shape) - 1)
    return volume((1000.0 + 0.005 * noise).astype(F))


def far_narrow_table():
    rows = [[0, 0]]
    for c in (0.4, 0.5, 0.6):
        rows += [[c - 0.01, 0], [c, 0.8], [c + 0.01, 0]]
    rows.append([1, 0])
    return TransferFunction(GRAY, np.array(rows, F), (1000.0, 1000.005))


# ---- outside: every value below value_lo, or above value_hi; the table is transparent at both ends
def outside(above):
    vol = volume(scenes.noise_volume(27, seed=9).data[:, :10, :19])
    t = TransferFunction(GRAY, np.array([[0, 0], [0.1, 0], [0.5, 1], [0.9, 0], [1, 0]], F), (-2.0, -1.0) if above else (2.0, 3.0))
    return vol, t


# ---- huge: finite +-3e38 neighbours; a lerp between them overflows
HUGE_VERTS = (((5, 4, 6), 3e38), ((6, 4, 6), -3e38), ((5, 5, 6), -3e38), ((12, 2, 20), -3e38), ((12, 2, 21), 3e38), ((18, 9, 26), 3e38),
              ((17, 9, 26), -3e38))


def huge():
    nx, ny, nz = COUNTS
    d = np.full((nz, ny, nx), 0.5, F)
    for (x, y, z), v in HUGE_VERTS:
        d[z, y, x] = v
    return volume(d)


def huge_table(where):
    """bottom / top over (0, 1); `low`: opaque at entry 0 only, over a value range that puts -3e38 at entry 30 and 0.5 at 255."""
    if where == "low":
        return TransferFunction(GRAY, np.array([[0, 1], [0.02, 0], [1, 0]], F), (-3.4e38, 0.0))
    return nonfinite_table(where)


# ---- thin and offset bricks
def thin(counts, seed=2):
    """A whole volume of these vertex counts (x y z), noise in [0, 1]."""
    nx, ny, nz = counts
    rng = np.random.default_rng(seed)
    return volume(rng.random((nz, ny, nx), dtype=np.float32))


def cut(vol, offset, counts):
    """The brick [offset, offset + counts) of vol's grid (scenes.split_volume's boxes, at any offset)."""
    off, cnt = np.array(offset, np.int32), np.array(counts, np.int32)
    org, sp = np.asarray(vol.origin, F), np.asarray(vol.spacing, F)
    d = np.ascontiguousarray(vol.data[off[2]:off[2] + cnt[2], off[1]:off[1] + cnt[1], off[0]:off[0] + cnt[0]])
    lo = (org + off.astype(F) * sp).astype(F)
    hi = (org + (off + cnt - 1).astype(F) * sp).astype(F)
    return scenes.Brick(d, off, vol.counts.copy(), org, sp, lo, hi)


# (A, B, union): B continues A along +z; the cuts fall on no multiple of 8.  The second pair's A is one cell thick
CHAINS = ((((3, 1, 5), (13, 8, 7)), ((3, 1, 11), (13, 8, 11)), ((3, 1, 5), (13, 8, 17))),
          (((1, 2, 9), (17, 7, 2)), ((1, 2, 10), (17, 7, 13)), ((1, 2, 9), (17, 7, 14))))


def chain(vol, which):
    return tuple(cut(vol, o, c) for o, c in CHAINS[which])


def hop(marched):
    """What gvt_hip_shuffle_volume hands to the next brick: (the selection, the rays that are not finished, RAY_BOUNDARY cleared)."""
    go = (marched["depth"] & vc.OPAQUE) == 0
    on = marched[go].copy()
    on["depth"] &= ~vc.BOUNDARY
    return go, on


def smooth():
    """Smooth noise on the shared geometry (the global grid the offset bricks are cut from)."""
    return volume(scenes.noise_volume(27, seed=6).data[:, :10, :19])


# ---- rays
def box(vol):
    lo = np.asarray(getattr(vol, "lo", vol.origin), F)
    if hasattr(vol, "hi"):
        return lo, np.asarray(vol.hi, F)
    return lo, (vol.origin + (vol.counts - 1).astype(F) * vol.spacing).astype(F)


def _rays(org, d, m, t_min=1e-6, w=0.0, color=(0, 0, 0)):
    M = np.asarray(m, F).reshape(4, 4).T
    r = np.zeros(len(org), RAY_DTYPE)
    with np.errstate(all="ignore"):
        r["origin"] = (np.asarray(org, F) @ M[:3, :3].T + M[:3, 3]).astype(F)
        r["direction"] = (np.asarray(d, F) @ M[:3, :3].T).astype(F)
    r["t_min"] = np.asarray(t_min, F)
    r["t_max"] = np.finfo(F).max
    r["w"] = np.asarray(w, F)
    r["color"] = np.asarray(color, F)
    return r


def _aimed(rng, lo, hi, n, inside=0.3):
    """Origins around and inside the box, aimed at a point inside it (the direction is not normalised: t = 1 is the target)."""
    ext = hi - lo
    org = (lo - 0.5 * ext + 2.0 * ext * rng.random((n, 3))).astype(F)
    ins = rng.random(n) < inside
    org[ins] = (lo + ext * rng.random((int(ins.sum()), 3))).astype(F)
    tgt = (lo + ext * rng.random((n, 3))).astype(F)
    return org, (tgt - org).astype(F)


def edge_rays(vol, m, rate=1.0, seed=13):
    """About 2,000 rays in world space: make_rays' five groups, then origins exactly on faces, edges and corners (aimed inwards, and
    running along the face or edge: the zero direction component at o == lo and at o == hi), rays through grid vertices, zero, NaN and Inf
    directions and origins, t_min negative / exactly on the lattice / 1e30 / beyond the exit, and rays that arrive almost or already
    opaque with a colour.  One fixed permutation interleaves long and dead rays inside a wave.  id = the position before it."""
    rng = np.random.default_rng(seed)
    lo, hi = box(vol)
    sp = np.asarray(vol.spacing, F)
    dt = F(F(min(sp)) / F(rate))
    ext = hi - lo
    parts = [make_rays(vol, m, n=1000, seed=5)]
    # origins on lo / hi faces, edges and corners
    org, d = [], []
    for code in range(27):
        pin = [(code // 3 ** a) % 3 for a in range(3)]  # 0: free, 1: lo, 2: hi
        if not any(pin):
            continue
        for rep in range(10):
            o = (lo + ext * rng.random(3)).astype(F)
            for a in range(3):
                if pin[a]:
                    o[a] = lo[a] if pin[a] == 1 else hi[a]
            t = (lo + ext * rng.random(3)).astype(F)
            dd = (t - o).astype(F)
            if rep >= 6:  # along the face / edge; a corner keeps one axis
                keep = rep % 3
                for a in range(3):
                    if pin[a] and not (all(pin) and a == keep):
                        dd[a] = 0
                s = float(np.abs(dd / ext).max())  # (no |d| far below the spacing: such a ray walks thousands of lattice steps)
                if 0 < s < 0.3:
                    dd = (dd * F(0.5 / s)).astype(F)
            org.append(o)
            d.append(dd)
    parts.append(_rays(np.array(org), np.array(d), m))
    # through grid vertices: whole and half cell steps per lattice step
    n = 300
    cnt = np.asarray(vol.counts)
    off = np.asarray(getattr(vol, "offset", np.zeros(3)), np.int64)
    v = off + (rng.random((n, 3)) * cnt).astype(np.int64)
    step = rng.integers(-3, 4, (n, 3))
    step[(step == 0).all(axis=1)] = (1, 0, -1)
    half = np.where(rng.random(n) < 0.5, 0.5, 1.0)[:, None]
    cell = (step * half * sp).astype(F)                      # exact: dyadic
    back = rng.integers(0, 40, n)[:, None]
    vpos = (np.asarray(vol.origin, F) + v.astype(F) * sp).astype(F)
    parts.append(_rays((vpos - back.astype(F) * cell).astype(F), (cell / dt).astype(F), m))
    # zero / NaN / Inf
    org, d = _aimed(rng, lo, hi, 40)
    d[:8] = 0
    for i in range(8, 40):
        which, a = (i - 8) // 3 % 4, (i - 8) % 3
        if which == 0:
            org[i, a] = np.nan
        elif which == 1:
            d[i, a] = np.nan
        elif which == 2:
            org[i, a] = np.inf if i % 2 else -np.inf
        else:
            d[i, a] = np.inf if i % 2 else -np.inf
    parts.append(_rays(org, d, m))
    # t_min
    org, d = _aimed(rng, lo, hi, 200)
    t_min = np.empty(200, F)
    t_min[:50] = -rng.random(50).astype(F) * 2
    t_min[50:150] = rng.integers(0, 60, 100).astype(F) * dt  # exactly on the lattice
    t_min[150:170] = 1e30
    t_min[170:] = 50.0
    parts.append(_rays(org, d, m, t_min))
    # incoming opacity and colour
    org, d = _aimed(rng, lo, hi, 180)
    w = np.repeat(np.array([0.98999, 0.99, 1.0], F), 60)
    parts.append(_rays(org, d, m, 1e-6, w, (0.2, 0.3, 0.1)))
    r = np.concatenate(parts)
    r["id"] = np.arange(len(r))
    r["depth"] = 0
    return r[np.random.default_rng(99).permutation(len(r))]


def chain_rays(a, b, m, n=900, seed=17):
    """Rays that cross brick a and then brick b (never b first; b continues a along +z): from below or inside a towards a point in b,
    most of them through both."""
    rng = np.random.default_rng(seed)
    lo, hi = np.minimum(a.lo, b.lo), np.maximum(a.hi, b.hi)
    ext = hi - lo
    org = (lo - 0.1 * ext + 1.2 * ext * rng.random((n, 3))).astype(F)
    org[:, 2] = (a.lo[2] - 0.3 * (a.hi[2] - a.lo[2]) + 1.2 * (a.hi[2] - a.lo[2]) * rng.random(n)).astype(F)
    tgt = (lo + ext * rng.random((n, 3))).astype(F)
    tgt[:, 2] = (b.lo[2] + (b.hi[2] - b.lo[2]) * rng.random(n)).astype(F)
    r = _rays(org, (tgt - org).astype(F), m)
    r["id"] = np.arange(n)
    return r


# ---- what the host test measures with the checker's own pieces
def owned_samples(B, rays, minv):
    """Every lattice sample brick B owns along the rays' lines (no early termination), with the checker's range, ownership and
    interpolation: arrays ray, k, cell (n, 3), value."""
    with np.errstate(all="ignore"):
        o = vc.xfm_point(minv, rays["origin"])
        d = vc.xfm_vector(minv, rays["direction"])
    tn, tf = vc.slab(B.lo, B.hi, o, d)
    kp = vc.first_after(rays["t_min"], B.dt)
    with np.errstate(all="ignore"):
        qlo, qhi = np.floor(tn / B.dt), np.floor(tf / B.dt)
        ok = (tn <= tf) & (tf >= 0) & (tf < np.inf) & (kp >= 0) & (qlo < vc.K_MAX)
        kb = np.where(qlo > 1, np.nan_to_num(qlo, neginf=0, posinf=0).astype(np.int64) - 1, 0)
        qh = np.nan_to_num(qhi, neginf=0, posinf=0).astype(np.int64)
    k0 = np.where(ok, np.maximum(kp, kb), 0)
    k1 = np.where(ok, qh + 1, -1)
    nx, ny = int(B.n[0]), int(B.n[1])
    flat = B.vox.reshape(-1)
    out = [[], [], [], []]
    idx = np.nonzero(ok)[0]
    assert (k1[idx] - k0[idx]).max(initial=0) < 5000
    for s in range(int((k1[idx] - k0[idx]).max(initial=-1)) + 1):
        j = idx[k0[idx] + s <= k1[idx]]
        k = k0[j] + s
        own, c, f = vc.cells(B, o[j], d[j], k)
        j, k, c, f = j[own], k[own], c[own], f[own]
        base = c[:, 0] + nx * c[:, 1] + nx * ny * c[:, 2]
        sy, sz = nx, nx * ny
        with np.errstate(all="ignore"):
            c00, c10 = vc.lerp(flat[base], flat[base + 1], f[:, 0]), vc.lerp(flat[base + sy], flat[base + sy + 1], f[:, 0])
            c01, c11 = vc.lerp(flat[base + sz], flat[base + sz + 1], f[:, 0]), vc.lerp(flat[base + sz + sy], flat[base + sz + sy + 1], f[:, 0])
            v = vc.lerp(vc.lerp(c00, c10, f[:, 1]), vc.lerp(c01, c11, f[:, 1]), f[:, 2])
        for lst, x in zip(out, (j, k, c, v)):
            lst.append(x)
    return tuple(np.concatenate(x) if x else np.zeros((0, 3) if i == 2 else 0, np.int64) for i, x in enumerate(out))


def opacity_at(B, v):
    """The corrected opacity the checker's look-up gives value v."""
    with np.errstate(all="ignore"):
        pos = np.fmin(np.fmax((v - B.vlo) / B.vspan, F(0)), F(1)) * F(255)
        i0 = np.minimum(pos.astype(np.int64), 254)
        w = (pos - i0.astype(F)).astype(F)
        return vc.lerp(B.tf[i0, 3], B.tf[i0 + 1, 3], w).astype(F)


def candidate_empty_blocks(B):
    """(nbz, nby, nbx) bool: macro cells whose vertices are all finite and all map to table entries of zero opacity -- a plain min / max
    per block, not the library's rule."""
    nb = [(int(n) - 1 + 7) // 8 for n in B.n]
    out = np.zeros((nb[2], nb[1], nb[0]), bool)
    for bz in range(nb[2]):
        for by in range(nb[1]):
            for bx in range(nb[0]):
                v = B.vox[8 * bz:8 * bz + 9, 8 * by:8 * by + 9, 8 * bx:8 * bx + 9]
                if not np.isfinite(v).all():
                    continue
                p = np.clip((np.array([v.min(), v.max()], np.float64) - float(B.vlo)) / float(B.vspan), 0, 1) * 255
                e0, e1 = int(np.floor(p[0])), min(int(np.floor(p[1])) + 1, 255)
                out[bz, by, bx] = (B.tf[e0:e1 + 1, 3] == 0).all()
    return out


def rays_through_empty_blocks(B, rays, minv):
    """Rays that own a sample in a candidate-empty block before their first sample anywhere else (so the march certainly reaches it),
    and the candidate mask."""
    cand = candidate_empty_blocks(B)
    j, k, c, _ = owned_samples(B, rays, minv)
    in_cand = cand[c[:, 2] >> 3, c[:, 1] >> 3, c[:, 0] >> 3]
    first_other = np.full(len(rays), np.iinfo(np.int64).max)
    np.minimum.at(first_other, j[~in_cand], k[~in_cand])
    fresh = rays["w"][j] < vc.OPAQUE_A
    return np.unique(j[in_cand & fresh & (k < first_other[j])]), cand


# the dataset / table pairs of the skip-exactness tests: name -> (volume, table, must_skip)
def skip_cases():
    cases = {}
    for e in PLATEAU_SPIKES:
        cases["plateaus-%d" % e] = (plateaus(), spike(e), True)
    for e in (81, 82, 177):
        cases["plateaus_half-%d" % e] = (plateaus(True), spike(e), True)
    for kind in ("pinf", "ninf", "nan", "mixed"):
        for where in ("bottom", "top", "middle"):
            cases["nonfinite-%s-%s" % (kind, where)] = (nonfinite(kind), nonfinite_table(where), where != "middle")
    cases["far_narrow"] = (far_narrow(), far_narrow_table(), True)
    for above in (False, True):
        cases["outside-%s" % ("above" if above else "below")] = outside(above) + (True,)
    for where in ("bottom", "top", "low"):
        cases["huge-%s" % where] = (huge(), huge_table(where), True)
    return cases
