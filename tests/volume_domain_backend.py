"""A numpy backend for scheduler.VolumeDomainTracer (HipVolumeBackend's method names) built on tests/volume_checker.py: march, shuffle,
next_brick, camera_rays.  It exchanges CPU tensors, so the Domain scheduler's control flow over volume bricks runs without a device --
and gives the GPU tests the rounds and the rays sent of a case.  Also here: the threads-on-FakeWorld driver both test files use, and the
hop count of a frame taken from the checker's own shuffle.  A helper, not a test."""
import threading

import numpy as np
import torch

from gravit_amd import scenes
from gravit_amd.layouts import RAY_DTYPE
from gravit_amd.scheduler import VolumeDomainTracer, _brick_boxes
from oracle import orc
from tests import volume_checker as vc
from tests.fake_dist import FakeWorld

F = np.float32
IDENT = scenes.mat_translate_scale((0, 0, 0), (1, 1, 1))


class NumpyVolumeBackend:
    def __init__(self, bricks, camera, tf, m=None, sampling_rate=1.0, owned=None):
        self.camera = camera
        self.m = np.asarray(IDENT if m is None else m, F).reshape(16)
        self.minv = scenes.instance_matrices(self.m)[0]
        self.n_inst = len(bricks)
        self.owned = [True] * self.n_inst if owned is None else [bool(o) for o in owned]
        self.bricks = [vc.Brick(b, tf, sampling_rate) if self.owned[i] else None for i, b in enumerate(bricks)]
        self.lo, self.hi = _brick_boxes(bricks, self.m)
        self.order = orc.toplevel_order(self.lo, self.hi)
        self.fb = np.zeros((camera.width * camera.height, 4), F)
        self.queues = [[] for _ in range(self.n_inst)]
        self.calls = 0

    def begin_frame(self):
        self.fb[:] = 0
        self.queues = [[] for _ in range(self.n_inst)]
        self.calls = 0

    def generate_and_filter(self, keep_mask=None):
        first = [[] for _ in range(self.n_inst)]
        vc.shuffle(self.lo, self.hi, self.order, vc.camera_rays(self.camera), -1, first, self.fb)
        for i in range(self.n_inst):
            if keep_mask is None or keep_mask[i]:
                self.queues[i] += first[i]

    def queue_sizes(self):
        return [sum(len(a) for a in q) for q in self.queues]

    def _take(self, inst):
        rays = np.concatenate(self.queues[inst]) if self.queues[inst] else np.zeros(0, RAY_DTYPE)
        self.queues[inst] = []
        return rays

    def trace_and_shuffle(self, inst):
        rays = vc.march(self.bricks[inst], self._take(inst), self.minv)
        self.calls += 1
        vc.shuffle(self.lo, self.hi, self.order, rays, inst, self.queues, self.fb)

    def export_wire(self, insts, torch, device):
        rays = np.concatenate([self._take(i) for i in insts]) if insts else np.zeros(0, RAY_DTYPE)
        return torch.from_numpy(np.ascontiguousarray(rays).view(F).reshape(-1, 20).copy())

    def append_wire(self, insts, buf, off, counts):
        rays = np.ascontiguousarray(buf.numpy()).reshape(-1).view(RAY_DTYPE)
        for i, n in zip(insts, counts):
            self.queues[i].append(rays[off:off + n].copy())
            off += n

    def fb_tensor(self, torch, device):
        return torch.from_numpy(self.fb.reshape(-1))

    def framebuffer(self, clamp=False):
        return np.minimum(self.fb, F(1)) if clamp else self.fb.copy()

    def sync(self):
        pass

    def stats(self):
        return {"adapter_calls": self.calls}


def hops(bricks, lo, hi, minv, cam):
    """The one-rank frame of volume_checker.frame with every shuffle's moves counted: (framebuffer (H, W, 4), moves[a][b] = rays that
    went from brick a to brick b, marched[a] = rays brick a marched).  The camera's own distribution (from -1) is not a hop."""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    n = len(bricks)
    fb = np.zeros((cam.width * cam.height, 4), F)
    queues = [[] for _ in range(n)]
    moves = np.zeros((n, n), np.int64)
    marched = np.zeros(n, np.int64)
    vc.shuffle(lo, hi, order, vc.camera_rays(cam), -1, queues, fb)
    while True:
        sizes = [sum(len(a) for a in q) for q in queues]
        if not any(sizes):
            break
        a = int(np.argmax(sizes))
        rays = vc.march(bricks[a], np.concatenate(queues[a]), minv)
        queues[a] = []
        marched[a] += len(rays)
        out = [[] for _ in range(n)]
        vc.shuffle(lo, hi, order, rays, a, out, fb)
        for b in range(n):
            moves[a, b] += sum(len(x) for x in out[b])
            queues[b] += out[b]
    return fb.reshape(cam.height, cam.width, 4), moves, marched


def run_ranks(world, make_tracer, frames=1, between=None, timeout=120):
    """`world` ranks as threads over tests/fake_dist.FakeWorld: make_tracer(rank, dist) -> a VolumeDomainTracer; every rank renders and
    composites `frames` times (between(tracer, k) runs before frame k > 0).  Returns {rank: [(image or None, rays_sent, rounds,
    adapter_calls, stats)] per frame}.  An exception in a rank aborts the barrier, so the others end too."""
    fw = FakeWorld(world)
    out, errs = {}, []

    def rank_main(rank):
        try:
            tr = make_tracer(rank, fw.rank_view(rank))
            res = []
            for k in range(frames):
                if k and between is not None:
                    between(tr, k)
                tr()
                img = tr.composite()
                res.append((img, tr.rays_sent, tr.rounds, tr.adapter_calls, tr.stats()))
            out[rank] = res
        except Exception:  # noqa: BLE001
            import traceback

            errs.append(traceback.format_exc())
            try:
                fw.barrier.abort()
            except Exception:  # noqa: BLE001
                pass

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=timeout) for t in th]
    assert not errs, errs[0]
    assert not any(t.is_alive() for t in th), "a rank did not end: the loop does not terminate"
    return out


def numpy_run(bricks, owner, world, cam, tf, rate, overlap=False, m=None):
    """The case on the numpy backend: {rank: [(image, rays_sent, rounds, adapter_calls, stats)]}."""
    def make(rank, dist):
        owned = [o == rank for o in owner]
        B = NumpyVolumeBackend(bricks, cam, tf, m, rate, owned)
        return VolumeDomainTracer(bricks, owner, cam, tf, dist, torch, torch.device("cpu"), m=m, sampling_rate=rate, backend=B, overlap=overlap)

    return run_ranks(world, make)


# ---- the cases both test files render: a 25^3 noise grid (3 macro cells per axis), sampling rate 1.3, a 48 x 36 film
RATE = 1.3
SPLITS = {"2x2x2": (2, 2, 2), "3x1x2": (3, 1, 2)}
EYES = {"outside": (1.55, 1.5, 1.75), "inside": (0.17, 0.57, -0.03)}  # inside: in one brick, a tenth of the grid from three brick faces


def case_volume(seed=3):
    n = 25
    vol = scenes.noise_volume(n, seed=seed)
    vol.origin = np.array([-0.25, 0.1, -0.4], F)
    vol.spacing = np.array([1.0 / (n - 1), 1.1 / (n - 1), 0.9 / (n - 1)], F)
    return vol


def case_camera(eye):
    return scenes.Camera(EYES[eye], (0.25, 0.65, 0.05), (0.0, 1.0, 0.0), float(F(40.0 * np.pi / 180.0)), 48, 36)


def case_tf(kind):
    """thin: no ray turns opaque.  dense: most rays end OPAQUE a brick or two behind the one they enter first."""
    import os

    from gravit_amd.adapter import TransferFunction
    from tests.conftest import GOLDEN

    cool = TransferFunction.read_map(os.path.join(GOLDEN, "colormaps", "CoolWarm.cmap"), 4)
    omap = {"thin": [[0, 0.01], [1, 0.08]], "dense": [[0, 0.1], [1, 0.5]]}[kind]
    return TransferFunction(cool, np.array(omap, F), (0.0, 1.0))


def case_owner(kind, bricks, world):
    """round_robin; checker: every face neighbour of a brick belongs to another rank; last: all bricks on the last rank."""
    if kind == "round_robin":
        return [i % world for i in range(len(bricks))]
    if kind == "last":
        return [world - 1] * len(bricks)
    axes = [sorted({int(b.offset[a]) for b in bricks}) for a in range(3)]
    return [sum(axes[a].index(int(b.offset[a])) for a in range(3)) % world for b in bricks]
