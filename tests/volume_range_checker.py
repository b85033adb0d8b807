"""numpy restatement of what a volume keeps per macro cell and of the n_blocks_empty rule, from the wording of include/gvt_hip.h
(gvt_hip_volume_update_samples, gvt_hip_volume_set_transfer): the value range of a macro cell's vertices, its not-finite flag, and
which macro cells a transfer function leaves empty.  No GPU here."""
import numpy as np

from tests import volume_checker as vc

F = np.float32


def blocks(counts):
    """Macro cells (8^3 cells each) per axis, for vertex counts per axis."""
    return [(int(c) - 1 + 7) // 8 for c in counts]


def ranges(data):
    """data[z, y, x] -> (bmin, bmax, wild), each (nbz, nby, nbx): per macro cell the minimum and maximum of its vertices that are not NaN
    (+Inf and -Inf where it has none) and whether one of its vertices is NaN or +-Inf.  A macro cell's vertices are those of its (up to)
    8^3 cells: 9 per axis, clipped at the brick's last vertex; a vertex on a block boundary counts for both blocks."""
    data = np.asarray(data, F)
    nbz, nby, nbx = blocks(data.shape)
    bmin = np.full((nbz, nby, nbx), np.inf, F)
    bmax = np.full((nbz, nby, nbx), -np.inf, F)
    wild = np.zeros((nbz, nby, nbx), bool)
    for bz in range(nbz):
        for by in range(nby):
            for bx in range(nbx):
                v = data[8 * bz:8 * bz + 9, 8 * by:8 * by + 9, 8 * bx:8 * bx + 9]
                num = v[~np.isnan(v)]
                if num.size:
                    bmin[bz, by, bx], bmax[bz, by, bx] = num.min(), num.max()
                wild[bz, by, bx] = not np.isfinite(v).all()
    return bmin, bmax, wild


def ranges_by_cells(data):
    """The same by brute force: every cell hands its 8 vertices to the macro cell it lies in."""
    data = np.asarray(data, F)
    nz, ny, nx = data.shape
    nbz, nby, nbx = blocks(data.shape)
    bmin = np.full((nbz, nby, nbx), np.inf, F)
    bmax = np.full((nbz, nby, nbx), -np.inf, F)
    wild = np.zeros((nbz, nby, nbx), bool)
    for cz in range(nz - 1):
        for cy in range(ny - 1):
            for cx in range(nx - 1):
                b = (cz // 8, cy // 8, cx // 8)
                for v in data[cz:cz + 2, cy:cy + 2, cx:cx + 2].reshape(-1):
                    if np.isnan(v):
                        wild[b] = True
                        continue
                    if np.isinf(v):
                        wild[b] = True
                    bmin[b] = min(bmin[b], v)
                    bmax[b] = max(bmax[b], v)
    return bmin, bmax, wild


def value_range(data):
    """value_min / value_max: over the samples that are not NaN (+Inf / -Inf with none)."""
    num = np.asarray(data, F)
    num = num[~np.isnan(num)]
    return (F(num.min()), F(num.max())) if num.size else (F(np.inf), F(-np.inf))


def empty_blocks(data, tf, sampling_rate=1.0):
    """(nbz, nby, nbx) bool: the macro cells gvt_hip_volume_set_transfer counts in n_blocks_empty.  With e(v) = floor(clamp((v - lo) /
    (hi - lo), 0, 1) * 255) in double, a macro cell is empty when no entry in [max(0, e(min) - 1), min(255, e(max) + 2)] has a positive
    corrected opacity; the interval starts at entry 0 when a vertex is not finite, and is the whole table when the cell has no vertex that
    is a number or when max - min (in double) reaches 3.4e38."""
    a = vc.table(tf.cmap, tf.omap, sampling_rate)[:, 3]
    lo, hi = float(F(tf.value_range[0])), float(F(tf.value_range[1]))
    bmin, bmax, wild = ranges(data)
    out = np.zeros(bmin.shape, bool)

    def entry(v):
        p = (float(v) - lo) / (hi - lo)
        return int(np.floor(min(max(p, 0.0), 1.0) * 255.0))

    for b in np.ndindex(bmin.shape):
        e0, e1 = 0, 255
        if bmin[b] <= bmax[b] and float(bmax[b]) - float(bmin[b]) < 3.4e38:
            e0 = 0 if wild[b] else max(0, entry(bmin[b]) - 1)
            e1 = min(255, entry(bmax[b]) + 2)
        out[b] = not (a[e0:e1 + 1] > 0).any()
    return out


def n_blocks_empty(data, tf, sampling_rate=1.0):
    return int(empty_blocks(data, tf, sampling_rate).sum())
