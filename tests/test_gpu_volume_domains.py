"""Volume domains across ranks on the device.  The GPU box has ONE MI355X, so the P ranks of VolumeDomainTracer run as P threads of one
process, each with its own HipVolumeBackend (queues and boxes for every brick, adapters for the bricks it owns, its own framebuffer), and
exchange real device wire buffers through tests/fake_dist.py, one lock around library calls (as tests/test_gpu_domain.py does for meshes).

The contract (include/gvt_hip.h, "volume domains across ranks"): at one sample per pixel rank 0's composited framebuffer, un-clamped,
equals the one-rank VolumeTracer frame and tests/volume_checker.frame as uint32 bits, for every owner map, world size and both loops,
and the bricks' counters sum to the one-rank frame's.  No tolerance is involved.  Then the four entry points on their own:
gvt_hip_volume_camera_filter, gvt_hip_volume_march_queue and the batched wire pair."""
import ctypes as C
import functools
import itertools
import threading

import numpy as np
import pytest
import torch

from gravit_amd import capi, scenes
from gravit_amd.adapter import HipVolumeAdapter, RayQueue, camera_generate, queues_append_wire, queues_export_wire
from gravit_amd.layouts import RAY_DTYPE
from gravit_amd.scheduler import HipVolumeBackend, VolumeDomainTracer, VolumeTracer
from tests import volume_amr_cases as amr_cases
from tests import volume_checker as vc
from tests import volume_domain_backend as vdb

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID, ERR_CAPACITY = -1, -3
COUNTERS = ("samples_marched", "samples_gathered", "crossings_rendered", "samples_shaded")
LOCK = threading.Lock()


class Locked:
    """libgvt_hip.so serialises work on one stream and shares scratch arenas: one thread inside it at a time."""

    def __init__(self, inner):
        self._b = inner

    def __getattr__(self, name):
        attr = getattr(self._b, name)
        if not callable(attr):
            return attr

        def call(*a, **k):
            with LOCK:
                return attr(*a, **k)
        return call


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def gpu_run(parts, owner, world, cam, tf, overlap, native=False, setup=None, frames=1, between=None):
    def make(rank, dist):
        owned = [o == rank for o in owner]
        with LOCK:
            B = HipVolumeBackend(parts, cam, tf, None, vdb.RATE, True, native, owned)
            assert [a is not None for a in B.adapters] == owned  # adapters only for the owned bricks
        tr = VolumeDomainTracer(parts, owner, cam, tf, dist, torch, torch.device("cuda", 0), sampling_rate=vdb.RATE, native=native,
                                backend=Locked(B), overlap=overlap)
        if setup is not None:
            setup(tr)
        return tr

    return vdb.run_ranks(world, make, frames, between)


def summed(res, world, frame=-1):
    return {k: sum(res[r][frame][4][k] for r in range(world)) for k in COUNTERS}


@functools.lru_cache(maxsize=None)
def reference(split, tf_kind, eye):
    """A case's bricks, camera and table; the one-rank VolumeTracer frame (bits and counters); the checker's frame and its hops."""
    parts = scenes.split_volume(vdb.case_volume(), *vdb.SPLITS[split])
    tf, cam = vdb.case_tf(tf_kind), vdb.case_camera(eye)
    one = VolumeTracer(parts, cam, tf, sampling_rate=vdb.RATE).frame()
    fb1, st1 = one.framebuffer(False), one.stats()
    minv = scenes.instance_matrices(vdb.IDENT)[0]
    bricks = [vc.Brick(b, tf, vdb.RATE) for b in parts]
    want, moves, marched = vdb.hops(bricks, [b.lo for b in parts], [b.hi for b in parts], minv, cam)
    return parts, cam, tf, fb1, st1, want, moves, marched


@functools.lru_cache(maxsize=None)
def numpy_counts(split, tf_kind, eye, owner_kind, world, overlap):
    parts, cam, tf = reference(split, tf_kind, eye)[:3]
    res = vdb.numpy_run(parts, vdb.case_owner(owner_kind, parts, world), world, cam, tf, vdb.RATE, overlap)
    return sum(res[r][0][1] for r in range(world)), [res[r][0][2] for r in range(world)]


# every bricking x world x owner map x loop; the four (table, eye) pairs take turns, so that each meets every value of every other axis
PAIRS = [("thin", "outside"), ("dense", "inside"), ("dense", "outside"), ("thin", "inside")]
CASES = [(split, world, owner_kind) + PAIRS[(k + k // 4) % 4] + (overlap,)
         for k, (split, world, owner_kind, overlap) in enumerate(itertools.product(("2x2x2", "3x1x2"), (2, 3, 8), ("round_robin", "checker", "last"), (False, True)))]


@pytest.mark.parametrize("split,world,owner_kind,tf_kind,eye,overlap", CASES)
def test_domains_equal_the_one_rank_frame_in_every_bit(hip, split, world, owner_kind, tf_kind, eye, overlap):
    parts, cam, tf, fb1, st1, want, moves, marched = reference(split, tf_kind, eye)
    assert (want[..., 3] != 0).mean() > 0.25  # a picture, not a blank film
    owner = vdb.case_owner(owner_kind, parts, world)
    res = gpu_run(parts, owner, world, cam, tf, overlap)
    img = res[0][0][0]
    assert (bits(img) == bits(fb1)).all() and (bits(img) == bits(want)).all()
    assert summed(res, world) == {k: st1[k] for k in COUNTERS}
    sent, rounds = numpy_counts(split, tf_kind, eye, owner_kind, world, overlap)
    assert sum(res[r][0][1] for r in range(world)) == sent
    assert sent > 0 or owner_kind == "last"  # (all bricks on one rank: nothing to send)
    assert sent == sum(moves[a, b] for a in range(len(owner)) for b in range(len(owner)) if owner[a] != owner[b])
    if not overlap:
        assert [res[r][0][2] for r in range(world)] == rounds
    for r in range(world):  # every rank that owns a brick the camera's rays reach marches
        if any(marched[i] for i in range(len(owner)) if owner[i] == r):
            assert res[r][0][3] >= 1
    if owner_kind == "last" and world > 1:  # rank 0 owns nothing and still composites
        assert res[0][0][3] == 0 and res[0][0][1] == 0


def one_rank(parts, cam, tf, native=False, setup=None):
    tr = VolumeTracer(parts, cam, tf, sampling_rate=vdb.RATE, native=native)
    if setup is not None:
        setup(tr)
    return tr


def surfaces(tr):  # an isovalue and a slice through the middle: the side mask crosses brick and rank boundaries
    tr.set_surfaces([0.5], [(0.3, 0.5, 1.0, 0.42)], 0.6).set_lights([((3.0, 4.0, 5.0), (1.0, 0.9, 0.8))])


def lit(tr):
    tr.set_lights([((3.0, 4.0, 5.0), (1.0, 0.9, 0.8)), ((-2.0, 1.0, 3.0), (0.3, 0.4, 0.6))]).set_shading(True)


@pytest.mark.parametrize("variant", ["surfaces", "lit", "uint8", "amr"])
def test_variants_equal_their_one_rank_frame(hip, variant):
    cam, tf = vdb.case_camera("outside"), vdb.case_tf("thin")
    native, setup = False, None
    if variant == "amr":
        parts = scenes.split_amr_volume(amr_cases.scene(), 2, 2, 2, cuts=amr_cases.CUTS)
    else:
        vol = vdb.case_volume()
        if variant == "uint8":
            vol = scenes.VolumeData(np.rint(vol.data * 255).astype(np.uint8), vol.origin, vol.spacing)
            tf = type(tf)(tf.cmap, tf.omap, (0.0, 255.0))
            native = True
        parts = scenes.split_volume(vol, 2, 2, 2)
        setup = {"surfaces": surfaces, "lit": lit}.get(variant)
    one = one_rank(parts, cam, tf, native, setup).frame()
    fb1, st1 = one.framebuffer(False), one.stats()
    assert (fb1[..., 3] != 0).mean() > 0.25
    owner = vdb.case_owner("checker", parts, 3)
    res = gpu_run(parts, owner, 3, cam, tf, False, native, setup)
    assert (bits(res[0][0][0]) == bits(fb1)).all()
    assert summed(res, 3) == {k: st1[k] for k in COUNTERS}
    assert sum(res[r][0][1] for r in range(3)) > 0
    if variant == "surfaces":
        assert st1["crossings_rendered"] > 0
    if variant == "lit":
        assert st1["samples_shaded"] > 0
    if variant == "amr":
        assert sum(res[r][0][4]["samples_refined"] for r in range(3)) == st1["samples_refined"] > 0


def test_update_to_a_second_time_step_then_another_frame(hip):
    cam, tf = vdb.case_camera("outside"), vdb.case_tf("thin")
    step = [scenes.split_volume(vdb.case_volume(seed), 2, 2, 2) for seed in (3, 11)]
    one = one_rank(step[0], cam, tf).frame()
    fb_a = one.framebuffer(False)
    fb_b = one.update(step[1]).frame().framebuffer(False)
    assert (bits(fb_a) != bits(fb_b)).any()
    owner = vdb.case_owner("round_robin", step[0], 2)
    res = gpu_run(step[0], owner, 2, cam, tf, True, frames=2, between=lambda tr, k: tr.update(step[k]))
    assert (bits(res[0][0][0]) == bits(fb_a)).all() and (bits(res[0][1][0]) == bits(fb_b)).all()
    assert summed(res, 2) == {k: one.stats()[k] for k in COUNTERS}  # (the counters run over both frames on both sides)


# ---- gvt_hip_volume_camera_filter
def camera_step(B):
    """The camera step of gvt_hip_volume_frame, spelled out: the tiled camera list shuffled from -1."""
    q_cam = RayQueue()
    camera_generate(q_cam, B.camera, tile=8)
    queues = [RayQueue() for _ in range(B.n_inst)]
    arr = (C.c_void_p * B.n_inst)(*[q.h for q in queues])
    capi.check(capi.load().gvt_hip_shuffle_volume(B.top.h, q_cam.h, -1, arr, B.fb.h), "gvt_hip_shuffle_volume")
    return [q.to_numpy() for q in queues]


def raw(rays):
    return np.ascontiguousarray(rays).view(np.uint8).reshape(-1, 80)


@pytest.mark.parametrize("eye", ["outside", "inside"])
def test_camera_filter_keeps_the_frames_rays_in_their_order(hip, eye):
    parts = scenes.split_volume(vdb.case_volume(), 2, 2, 2)
    B = HipVolumeBackend(parts, vdb.case_camera(eye), vdb.case_tf("thin"), sampling_rate=vdb.RATE)
    want = camera_step(B)
    assert sum(len(w) for w in want) > 48 * 36 // 4
    B.begin_frame()
    B.generate_and_filter(None)  # NULL keeps everything
    for q, w in zip(B.queues, want):
        assert (raw(q.to_numpy()) == raw(w)).all()
    for keep in ([1, 0, 0, 1, 0, 1, 1, 0], [0] * 7 + [1], [0] * 8):
        B.begin_frame()
        B.generate_and_filter(np.array(keep, np.uint8))
        for k, q, w in zip(keep, B.queues, want):
            got = q.to_numpy()
            assert len(got) == (len(w) if k else 0)
            assert (raw(got) == raw(w[:len(got)])).all()
    assert float(np.abs(B.framebuffer()).sum()) == 0.0  # a camera ray deposits nothing
    lib = capi.load()
    assert lib.gvt_hip_volume_camera_filter(None, None, None, None) == ERR_INVALID


# ---- gvt_hip_volume_march_queue
def test_march_queue_gives_the_bits_of_volume_trace(hip):
    vol = vdb.case_volume()
    tf, cam = vdb.case_tf("thin"), vdb.case_camera("outside")
    ad = HipVolumeAdapter(vol, sampling_rate=vdb.RATE)
    ad.set_transfer(tf)
    rays = vc.camera_rays(cam)
    rays = rays[::3].copy()
    rays["color"], rays["w"], rays["depth"] = 0, 0, 0  # as the shuffle from -1 hands them to a brick: no colour, no opacity, no flags
    q = RayQueue()
    q.append(rays, keep_state=True)
    ad.march_queue(q, vdb.IDENT)
    got = q.to_numpy()
    want = ad.trace(rays, vdb.IDENT, vdb.IDENT)
    assert len(got) == len(rays) and (raw(got) == raw(want)).all() and (got["w"] > 0).sum() > len(rays) // 4
    # rays clipped at their t_max: honoured with the flag, ignored without it (the CLIP = false launch, as in gvt_hip_volume_frame)
    clipped = rays.copy()
    clipped["depth"][::2] |= capi.RAY_CLIP
    clipped["t_max"][::2] = F(2.4)
    q.clear()
    q.append(clipped, keep_state=True)
    ad.march_queue(q, vdb.IDENT, may_clip=True)
    got_c = q.to_numpy()
    want_c = ad.trace(clipped, vdb.IDENT, vdb.IDENT)
    assert (raw(got_c) == raw(want_c)).all()
    assert (bits(got_c["w"]) != bits(got["w"])).any() and (bits(got_c["w"][1::2]) == bits(got["w"][1::2])).all()
    q.clear()
    q.append(clipped, keep_state=True)
    ad.march_queue(q, vdb.IDENT)
    assert (bits(q.to_numpy()["w"]) == bits(got["w"])).all()
    # refusals change nothing
    lib = capi.load()
    minv = capi.f32(vdb.IDENT, 16)
    before = q.to_numpy()
    bare = HipVolumeAdapter(vol, sampling_rate=vdb.RATE)  # no transfer function
    for args in ((None, q.h, capi.ptr(minv), 0), (ad.h, None, capi.ptr(minv), 0), (ad.h, q.h, None, 0), (ad.h, q.h, capi.ptr(minv), 2),
                 (bare.h, q.h, capi.ptr(minv), 0)):
        assert lib.gvt_hip_volume_march_queue(*args) == ERR_INVALID
    assert (raw(q.to_numpy()) == raw(before)).all()


# ---- the batched wire pair
def random_rays(n, seed):
    """n rays of random bytes (every bit pattern must survive the wire, NaNs included)."""
    return np.random.default_rng(seed).integers(0, 256, (n, 80), dtype=np.uint8).view(RAY_DTYPE).reshape(-1)


def sparse(n, at):
    sizes = [0] * n
    for k, v in at.items():
        sizes[k] = v
    return sizes


@pytest.mark.parametrize("sizes", [[0], [1], [65], [257], [0, 1, 65, 257], [257, 0, 0, 65, 1, 0, 64, 256], sparse(256, {3: 65, 100: 257, 255: 1}),
                                   sparse(256, {})], ids=lambda s: "n%d_%d" % (len(s), sum(s)))
def test_wire_pair_equals_the_per_queue_calls(hip, sizes):
    n, total = len(sizes), sum(sizes)
    rays = [random_rays(s, 17 + i) for i, s in enumerate(sizes)]
    queues = [RayQueue() for _ in range(n)]
    for q, r in zip(queues, rays):
        if len(r):
            q.append(r, keep_state=True)
    dev = torch.device("cuda", 0)
    want = torch.zeros((max(total, 1), 80), dtype=torch.uint8, device=dev)
    off = 0
    for q, s in zip(queues, sizes):  # the per-queue exports laid end to end
        if s:
            assert q.export_device(want.data_ptr() + off * 80, s) == s
        off += s
    lib = capi.load()
    arr = (C.c_void_p * n)(*[q.h for q in queues])
    got = torch.full((max(total, 1) + 1, 80), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    if total:  # the capacity refusal changes nothing and reports the need
        need, counts = C.c_uint64(0), (C.c_uint64 * n)()
        assert lib.gvt_hip_queues_export_wire(arr, n, C.c_void_p(got.data_ptr()), total - 1, counts, C.byref(need)) == ERR_CAPACITY
        assert need.value == total and [len(q) for q in queues] == sizes
        capi.synchronize()
        assert bool((got == 0xA5).all())
    assert queues_export_wire(queues, got.data_ptr(), total) == sizes
    assert [len(q) for q in queues] == [0] * n  # cleared
    host = got.cpu().numpy()
    assert (host[:total] == want.cpu().numpy()[:total]).all() and (host[total:] == 0xA5).all()  # ... and not a byte beyond
    if total:
        assert (host[:total] == np.concatenate([raw(r) for r in rays])).all()
    queues_append_wire(queues, got.data_ptr(), sizes)  # append after export restores the queues
    assert [len(q) for q in queues] == sizes
    for q, r in zip(queues, rays):
        assert (raw(q.to_numpy()) == raw(r)).all()
    queues_append_wire(queues, got.data_ptr(), sizes)  # ... and behind what a queue holds, like gvt_hip_queue_append(..., 1)
    twin = [RayQueue() for _ in range(n)]
    off = 0
    for t, r, s in zip(twin, rays, sizes):
        if s:
            t.append(r, keep_state=True)
            t.append_device(got.data_ptr() + off * 80, s)
        off += s
    for q, t in zip(queues, twin):
        assert len(q) == len(t) and (raw(q.to_numpy()) == raw(t.to_numpy())).all()


def test_wire_pair_refuses_null_arguments(hip):
    lib = capi.load()
    q = RayQueue()
    q.append(random_rays(5, 1), keep_state=True)
    arr = (C.c_void_p * 2)(q.h, None)
    one = (C.c_void_p * 1)(q.h)
    total, cnt = C.c_uint64(0), (C.c_uint64 * 2)(5, 0)
    buf = torch.zeros((8, 80), dtype=torch.uint8, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    assert lib.gvt_hip_queues_export_wire(None, 1, p, 8, None, C.byref(total)) == ERR_INVALID
    assert lib.gvt_hip_queues_export_wire(one, 1, p, 8, None, None) == ERR_INVALID
    assert lib.gvt_hip_queues_export_wire(arr, 2, p, 8, None, C.byref(total)) == ERR_INVALID  # a null queue
    assert lib.gvt_hip_queues_export_wire(one, 0, p, 8, None, C.byref(total)) == ERR_INVALID
    assert lib.gvt_hip_queues_export_wire(one, 257, p, 8, None, C.byref(total)) == ERR_INVALID
    assert lib.gvt_hip_queues_export_wire(one, 1, None, 8, None, C.byref(total)) == ERR_INVALID  # rays, and nowhere to put them
    assert lib.gvt_hip_queues_append_wire(None, 1, p, cnt) == ERR_INVALID
    assert lib.gvt_hip_queues_append_wire(one, 1, p, None) == ERR_INVALID
    assert lib.gvt_hip_queues_append_wire(arr, 2, p, cnt) == ERR_INVALID
    assert lib.gvt_hip_queues_append_wire(one, 1, None, cnt) == ERR_INVALID
    assert len(q) == 5 and (raw(q.to_numpy()) == raw(random_rays(5, 1))).all()
