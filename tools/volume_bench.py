"""Volume frame timing (not bench.py): a 1080p frame of scenes.noise_volume at 256^3 and 512^3, as one brick and as 8 bricks, through
gvt_hip_volume_frame.  Reports ms per frame (host clock around frames that end in a synchronisation), lattice samples per second, and the
voxel bytes per sample by the algorithmic count (8 reads of 4 bytes per interpolated sample, none for samples in skipped macro cells).
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (k_volume_march); counters in a run of their own.

  python tools/volume_bench.py [--sizes 256 512] [--steps 10] [--warmup 2] [--json OUT]
  python tools/volume_bench.py --dtype u8    (or i16, u16; every mode) the noise grid quantised with np.rint to the type's range and stored at
                                             that width (HipVolumeAdapter(native=True)), the transfer function's value range and the
                                             isovalues scaled to match; f32 (the default): the float grid, as before
  python tools/volume_bench.py --update      time-varying volumes: per grid size, with the samples in host memory and in device memory, the
                                             wall time of destroy + create + set_transfer (what a new time step cost before
                                             gvt_hip_volume_update_samples) and of the in-place update, its ms_out and where that goes: the
                                             range kernels (gvt_hip_profile's build class), ranges + download (an update of a volume without
                                             a transfer function), the rest = the host table rebuild and its upload.  --recreate-only: the
                                             first of these alone (it needs nothing the update added, so it also runs on an older tree)
  python tools/volume_bench.py --update --amr   time-varying AMR volumes: two time steps of the --fused --amr scene (256^3, the central eighth
                                             refined, ten subgrids) pushed alternately into one brick under the sparse table, samples in host
                                             and in device memory: the wall time of the three-call route (set_subgrids([]), update_samples,
                                             set_subgrids) and of gvt_hip_volume_update_amr, its ms_out and where that goes (range kernels,
                                             ranges + download, the host table rebuild; wall - ms_out = the uploads).  --three-call-only: the
                                             first of these alone (it needs nothing the in-place call added, so it also runs on an older tree)
  python tools/volume_bench.py --surfaces    the "thin" frames plain, with two isovalues the field never reaches (the per-sample cost of
                                             the side test alone) and with two it does (opacity 0.3, one light), each against the plain frame
  python tools/volume_bench.py --clip        geometry inside the volume: per grid size and bricking the "thin" frame plain and clipped at a depth
                                             plane that is +Inf everywhere (the same rays and samples: what the clip itself costs), frames
                                             alternating in one process; then the mixed frame -- bun_zipper inside the grid
                                             (scheduler.MixedTracer) -- and its parts: mesh frame, depth pass, clipped volume frame, composite
  python tools/volume_bench.py --shade --gradient central   smooth gradients: per grid size, table and bricking the lit frame and the
                                             isosurface frame with the CELL and with the CENTRAL gradient, alternating; the ratio
  python tools/volume_bench.py --shade       lit volumes: per grid size, table and bricking the frame unlit, lit by one light and lit by three
                                             (VolumeTracer.set_shading), frames alternating in one process on one tracer; with each the
                                             samples shaded per frame
  python tools/volume_bench.py --amr         AMR volumes: 1080p frames of the 256^3 noise grid at rate 2 under the "thin" table, frames
                                             alternating in one process: (a) the plain volume, (b) the same with an empty set of subgrids
                                             (the plain path), (c) one ratio-2 subgrid over the central eighth, (d) as (c) plus a ratio-4
                                             child over the subgrid's central eighth; then (e) the uniform 512^3 grid (c) would need, for
                                             memory and time beside it.  --sizes N: another level-0 size ((e) is 2 N)
  python tools/volume_bench.py --amr --surfaces   (and / or --amr --shade) shaded AMR volumes (GVT_HIP_VOLUME_AMR_SHADED): grid, subgrids,
                                             table and rate of (d) above; three frames alternating in one process: the AMR volume with two
                                             isovalues and a light (--surfaces) or lit by one light (--shade), the same level-0 volume without
                                             subgrids under the same surfaces / shading, and the plain AMR frame; the two ratios beside them
  python tools/volume_bench.py --fused --amr [--surfaces] [--shade] --bricks 1 8 64   the fused AMR frame (gvt_hip_volume_frame_fused_amr):
                                             grid, table and rate of (d) above, the central eighth refined as eight level-1 subgrids cut
                                             along the 4 x 4 x 4 brick faces (each lies in one brick of every bricking) with a ratio-4 child
                                             in two of them; per bricking three tracers alternating frame by frame in one process: the loop,
                                             the fused AMR frame, and the fused frame of the same level-0 grid without subgrids; median
                                             [min .. max] of each, the loop's and the fused framebuffer compared in every bit once.  Without
                                             --surfaces / --shade: the fog frame
  python tools/volume_bench.py --fused --amr --surfaces --shade --shadows [--fog-shadows] [--mesh-shadows] --bricks 1 8 64   shadows on AMR
                                             bricks (GVT_HIP_VOLUME_ALLOW_AMR): the same scene; per bricking and frame two tracers alternating
                                             frame by frame in one process -- the shadowed (fog-shadowed, mesh-shadowed) frame over the AMR
                                             bricks and the same frame over the same level-0 grid without subgrids -- and both tracers' bakes
                                             (--fog-shadows: the light grids; --mesh-shadows: the occluder grids, the bunny inside the grid)
  python tools/volume_bench.py --domains 1 2 4 8   volume domains across ranks: the "thin" 1080p frame of the 256^3 grid in 8 and in 64 bricks
                                             (round-robin owners) through scheduler.VolumeDomainTracer, W ranks as W threads of this process on
                                             ONE GPU over the stand-in transport of tests/fake_dist.py, one lock around library calls.  Per W and
                                             bricking: frame time (all ranks, composite included), rounds, rays sent, adapter calls, and the share
                                             of the frame the slowest rank spent in export + transfer + append; beside it the one-rank
                                             VolumeTracer.frame() (W = 1 against it prices the Python loop) and, with --per-queue, the same
                                             frames exchanging through one gvt_hip_queue_export / _append call per brick.  W > 1 on one GPU
                                             SHARES the device: this measures the protocol's overhead, not scaling
  python tools/volume_bench.py --fused       the fused frame (gvt_hip_volume_frame_fused): per grid size, table and bricking (1, 8 and 64
                                             bricks; --bricks to choose) the loop frame and the fused frame alternating frame by frame on ONE
                                             tracer in one process: median [min .. max] of each, brick visits, samples per second; "fused_wins" only
                                             where the fused maximum lies below the loop's minimum
  python tools/volume_bench.py --fused --surfaces   (and / or --shade) the shaded fused frame (gvt_hip_volume_frame_fused_shaded) against the loop,
                                             the same protocol: --surfaces = the "thin" frame with the two isovalues the field reaches (opacity
                                             0.3, one light), --shade = lit fog by one light under every --tf table; with each the crossings
                                             and the samples shaded per frame, and the two framebuffers compared bitwise after every pair
  python tools/volume_bench.py --fused --shade --fog-shadows  shadowed fog (gvt_hip_volume_frame_fog_shadowed): the lit fused frame, the same
                                                        frame with the fog shadowed from the light grids, and the bake
  python tools/volume_bench.py --fused --shade --fog-shadows --ao [--mesh-shadows] [--surfaces] [--gradient central]  ambient occlusion
                                             (gvt_hip_volume_frame_ao): per bricking the AO bake's ms beside the light grids' bake, the AO
                                             frame against its base frame in the same run, the brickings' framebuffers compared bitwise
  python tools/volume_bench.py --fused --shade --fog-shadows --mesh-shadows  meshes shadowing the volume (gvt_hip_volume_frame_mesh_shadowed):
                                                        the bunny of scenes.bunny_scene inside the grid (scenes.mesh_in_volume); the bake of the
                                                        occluder grids and its share spent in any-hit launches; the fog-shadowed frame and the
                                                        mesh-shadowed frame alternating frame by frame on ONE tracer; the brickings' framebuffers
                                                        compared bitwise.  With --surfaces also the frame with two isovalues, lit fog on and off
  python tools/volume_bench.py --fused ... --gradient central   ADDS, ahead of the rows the other flags print, the fused frames with CENTRAL
                                             bricks (GVT_HIP_FUSED_CENTRAL / GVT_HIP_VOLUME_ALLOW_CENTRAL): the lit and the isosurface frame,
                                             fused against the loop, per bricking; and for each of --shadows, --fog-shadows and --mesh-shadows
                                             (with the flags they go with, as ever) that shadowed frame with the CELL and with the CENTRAL
                                             gradient, alternating, from one bake.  All of them: --fused --surfaces --shade --shadows
                                             --fog-shadows --mesh-shadows --gradient central
  python tools/volume_bench.py --fused --surfaces --shadows   shadowed surfaces (gvt_hip_volume_frame_shadowed): --surfaces' frame shadowed
                                             against the same frame through the shaded fused kernel, alternating frame by frame on ONE
                                             tracer; with each the shadow rays and the shadow samples per frame, so that the cost per shadow
                                             sample stands beside the camera march's; the shadowed framebuffers of the brickings of one
                                             grid compared bitwise with each other ("same_bits_as_first": they must agree)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gravit_amd import _build, capi, scenes  # noqa: E402
from gravit_amd.adapter import TransferFunction  # noqa: E402
from gravit_amd.scheduler import VolumeTracer  # noqa: E402

F = np.float32
CMAPS = os.path.join(ROOT, "tests", "golden", "colormaps")


# --dtype: numpy dtype and the values the unit interval of noise_volume maps onto
DTYPES = {"f32": (np.float32, 0.0, 1.0), "u8": (np.uint8, 0.0, 255.0), "i16": (np.int16, -30000.0, 30000.0), "u16": (np.uint16, 0.0, 65535.0)}


def quantise(data, dtype):
    """The [0, 1] grid in the voxel type's units: rounded to the nearest integer for the integer types, untouched for f32."""
    np_t, lo, hi = DTYPES[dtype]
    if dtype == "f32":
        return data
    out = np.empty(data.shape, np_t)
    for z in range(data.shape[0]):  # slab by slab: no second float copy of a 512^3 grid
        out[z] = np.rint(data[z] * F(hi - lo) + F(lo)).astype(np_t)
    return out


def transfer(kind, dtype="f32"):
    """"thin": opacity rising linearly to 0.03 -- rays cross the whole grid, every sample is interpolated; "spikes": GraviT's
    fivespikes.omap -- opaque only around 0.9, most macro cells skipped.  The value range is the dtype's image of [0, 1]."""
    rd = TransferFunction.read_map
    cmap = rd(os.path.join(CMAPS, "CoolWarm.cmap"), 4)
    vr = DTYPES[dtype][1:]
    if kind == "thin":
        return TransferFunction(cmap, np.array([[0.0, 0.0], [1.0, 0.03]], F), vr)
    return TransferFunction(cmap, rd(os.path.join(CMAPS, "fivespikes.omap"), 2), vr)


def camera():
    return scenes.Camera((1.45, 1.1, 1.9), (0.5, 0.5, 0.5), (0.0, 1.0, 0.0), float(F(40.0 * np.pi / 180.0)), 1920, 1080)


SURFACE_MODES = {"plain": None, "never": (2.0, 3.0), "reached": (0.4, 0.6)}  # noise_volume lies in [0, 1]


def noise(n, dtype):
    vol = scenes.noise_volume(n, seed=1)
    vol.spacing = np.full(3, F(1.0 / (n - 1)), F)
    vol.data = quantise(vol.data, dtype)
    return vol


def run(n, split, steps, warmup, rate, kind, vol=None, surfaces=None, dtype="f32"):
    if vol is None:
        vol = noise(n, dtype)
    _, lo, hi = DTYPES[dtype]
    vbytes = np.dtype(DTYPES[dtype][0]).itemsize
    bricks = vol if split == (1, 1, 1) else scenes.split_volume(vol, *split)
    t0 = time.time()
    tr = VolumeTracer(bricks, camera(), transfer(kind, dtype), sampling_rate=rate, native=dtype != "f32")
    if surfaces:
        surfaces = tuple(lo + v * (hi - lo) for v in surfaces)
        tr.set_surfaces(surfaces, (), 0.3).set_lights([((3.0, 4.0, 5.0), (1.0, 1.0, 1.0))])
    setup = time.time() - t0
    for _ in range(warmup):
        tr.frame()
    s0 = tr.stats()
    capi.synchronize()
    times = []
    for _ in range(steps):
        t = time.perf_counter()
        tr.frame()
        capi.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    s1 = tr.stats()
    marched = (s1["samples_marched"] - s0["samples_marched"]) / steps
    gathered = (s1["samples_gathered"] - s0["samples_gathered"]) / steps
    ms = float(np.median(times))
    fb = tr.framebuffer(False)
    if surfaces:
        return {"n": n, "dtype": dtype, "tf": kind, "bricks": int(np.prod(split)), "isovalues": list(surfaces), "ms_median": round(ms, 3), "ms_min": round(min(times), 3),
                "ms_max": round(max(times), 3), "samples_per_frame": int(marched), "samples_interpolated": int(gathered),
                "crossings_per_frame": int((s1["crossings_rendered"] - s0["crossings_rendered"]) / steps), "lit_pixels": int((fb[..., 3] > 0).sum())}
    return {"n": n, "dtype": dtype, "tf": kind, "bricks": int(np.prod(split)), "split": list(split), "sampling_rate": rate, "ms_median": round(ms, 3),
            "ms_min": round(min(times), 3), "ms_max": round(max(times), 3), "adapter_calls": tr.calls,
            "samples_per_frame": int(marched), "samples_interpolated": int(gathered), "gsamples_per_s": round(marched / ms / 1e6, 3),
            "voxel_bytes_per_sample": round(8.0 * vbytes * gathered / max(marched, 1), 2), "voxel_bytes_per_frame_mb": round(8.0 * vbytes * gathered / 1e6, 1),
            "lit_pixels": int((fb[..., 3] > 0).sum()), "setup_s": round(setup, 1)}


def med(xs):
    return round(float(np.median(xs)), 3)


def timed(fn):
    t = time.perf_counter()
    fn()
    capi.synchronize()
    return (time.perf_counter() - t) * 1e3


def run_clip(n, split, steps, warmup, rate, vol, dtype="f32"):
    """The plain frame against the frame clipped at an all-+Inf plane, alternating."""
    from gravit_amd.adapter import DepthPlane

    bricks = vol if split == (1, 1, 1) else scenes.split_volume(vol, *split)
    cam = camera()
    tr = VolumeTracer(bricks, cam, transfer("thin", dtype), sampling_rate=rate, native=dtype != "f32")
    inf = DepthPlane(cam.width, cam.height)
    plain, clipped = [], []
    for i in range(warmup + steps):
        plain.append(timed(tr.frame))
        clipped.append(timed(lambda: tr.frame(inf)))
    plain, clipped = plain[warmup:], clipped[warmup:]
    return {"mode": "clip_inf", "n": n, "dtype": dtype, "bricks": int(np.prod(split)), "plain_ms_median": med(plain), "plain_ms_min": round(min(plain), 3),
            "plain_ms_max": round(max(plain), 3), "clipped_ms_median": med(clipped), "clipped_ms_min": round(min(clipped), 3), "clipped_ms_max": round(max(clipped), 3),
            "clipped_over_plain": round(float(np.median(clipped)) / float(np.median(plain)), 4)}


FUSED_SPLITS = {1: (1, 1, 1), 8: (2, 2, 2), 64: (4, 4, 4)}
SHADE_LIGHTS = [((3.0, 4.0, 5.0), (1.0, 0.9, 0.8)), ((-2.0, 1.0, 0.5), (0.2, 0.3, 0.4)), ((0.0, -6.0, 1.0), (0.5, 0.1, 0.3))]


def run_fused(n, split, steps, warmup, rate, kind, vol, dtype="f32", shaded=None):
    """The loop frame against the fused frame, alternating frame by frame on one tracer (VolumeTracer.fused switches the entry point).
    shaded: None (plain fog, gvt_hip_volume_frame_fused), "surfaces" (--surfaces' reached isovalues, opacity 0.3, one light) or "lit" (lit
    fog by --shade's first light): the shaded fused frame, its framebuffer compared with the loop's after every pair."""
    bricks = vol if split == (1, 1, 1) else scenes.split_volume(vol, *split)
    tr = VolumeTracer(bricks, camera(), transfer(kind, dtype), sampling_rate=rate, native=dtype != "f32", fused=True, fused_shaded=shaded is not None)
    if shaded == "surfaces":
        _, lo, hi = DTYPES[dtype]
        tr.set_surfaces(tuple(lo + v * (hi - lo) for v in SURFACE_MODES["reached"]), (), 0.3).set_lights([((3.0, 4.0, 5.0), (1.0, 1.0, 1.0))])
    elif shaded == "lit":
        tr.set_lights(SHADE_LIGHTS[:1]).set_shading(True)
    loop, fused = [], []
    pairs_same = True

    def frame(flag):
        tr.fused = flag
        tr.frame()

    for i in range(warmup + steps):
        loop.append(timed(lambda: frame(False)))
        loop_calls = tr.calls
        if shaded:
            a = tr.framebuffer(False).copy()
        fused.append(timed(lambda: frame(True)))
        if shaded:  # (outside the timed region)
            pairs_same = pairs_same and bool((a.view(np.uint32) == tr.framebuffer(False).view(np.uint32)).all())
    loop, fused = loop[warmup:], fused[warmup:]
    st = tr.stats()
    same = None
    if steps:  # (one more pair, compared: the two paths promise the same bits)
        frame(False)
        a = tr.framebuffer(False).copy()
        frame(True)
        same = pairs_same and bool((a.view(np.uint32) == tr.framebuffer(False).view(np.uint32)).all())
    extra = {}
    if shaded:
        extra = {"features": int(st["features"]), "crossings_per_frame": int(st["crossings_rendered"]), "samples_shaded": int(st["samples_shaded"])}
    return {"mode": "fused" if not shaded else "fused_" + shaded, **extra, "n": n, "dtype": dtype, "tf": kind, "bricks": int(np.prod(split)), "sampling_rate": rate, "loop_ms_median": med(loop),
            "loop_ms_min": round(min(loop), 3), "loop_ms_max": round(max(loop), 3), "loop_adapter_calls": int(loop_calls), "fused_ms_median": med(fused),
            "fused_ms_min": round(min(fused), 3), "fused_ms_max": round(max(fused), 3), "fused": int(st["fused"]), "brick_visits": int(st["brick_visits"]),
            "rays_deposited": int(st["rays_deposited"]), "samples_per_frame": int(st["samples_marched"]), "samples_interpolated": int(st["samples_gathered"]),
            "loop_gsamples_per_s": round(st["samples_marched"] / float(np.median(loop)) / 1e6, 3),
            "fused_gsamples_per_s": round(st["samples_marched"] / float(np.median(fused)) / 1e6, 3),
            "fused_over_loop": round(float(np.median(fused)) / float(np.median(loop)), 4), "fused_wins": bool(max(fused) < min(loop)), "same_bits": same}

def run_shadows(n, split, steps, warmup, rate, vol, dtype="f32", first=None, bias=2):
    """--surfaces' reached frame through the shaded fused kernel against the same frame shadowed, alternating frame by frame on one tracer
    (VolumeTracer.shadows switches the entry point).  first: the shadowed framebuffer of another bricking of the same grid, compared
    bitwise.  Returns (row, the shadowed framebuffer)."""
    bricks = vol if split == (1, 1, 1) else scenes.split_volume(vol, *split)
    tr = VolumeTracer(bricks, camera(), transfer("thin", dtype), sampling_rate=rate, native=dtype != "f32", fused=True, fused_shaded=True, shadow_bias=bias)
    _, lo, hi = DTYPES[dtype]
    tr.set_surfaces(tuple(lo + v * (hi - lo) for v in SURFACE_MODES["reached"]), (), 0.3).set_lights([((3.0, 4.0, 5.0), (1.0, 1.0, 1.0))])
    plain, shadowed = [], []

    def frame(flag):
        tr.shadows = flag
        tr.frame()

    for i in range(warmup + steps):
        plain.append(timed(lambda: frame(False)))
        ps = tr.stats()
        shadowed.append(timed(lambda: frame(True)))
    plain, shadowed = plain[warmup:], shadowed[warmup:]
    st = tr.stats()
    fb = tr.framebuffer(False).copy()
    extra_ms = float(np.median(shadowed)) - float(np.median(plain))
    row = {"mode": "fused_shadows", "n": n, "dtype": dtype, "tf": "thin", "bricks": int(np.prod(split)), "sampling_rate": rate, "bias": bias,
           "plain_ms_median": med(plain), "plain_ms_min": round(min(plain), 3), "plain_ms_max": round(max(plain), 3),
           "shadowed_ms_median": med(shadowed), "shadowed_ms_min": round(min(shadowed), 3), "shadowed_ms_max": round(max(shadowed), 3),
           "shadowed_over_plain": round(float(np.median(shadowed)) / float(np.median(plain)), 4), "shadowed": int(st["shadowed"]),
           "samples_per_frame": int(st["samples_marched"]), "samples_interpolated": int(st["samples_gathered"]), "crossings_per_frame": int(st["crossings_rendered"]),
           "camera_counters_same": bool(all(st[k] == ps[k] for k in ("samples_marched", "samples_gathered", "crossings_rendered", "brick_visits", "rays_deposited"))),
           "shadow_rays": int(st["shadow_rays"]), "shadow_brick_visits": int(st["shadow_brick_visits"]), "shadow_crossings": int(st["shadow_crossings"]),
           "shadow_samples": int(st["shadow_samples_marched"]), "shadow_samples_interpolated": int(st["shadow_samples_gathered"]),
           "plain_ns_per_sample": round(float(np.median(plain)) * 1e6 / max(st["samples_marched"], 1), 4),
           "extra_ns_per_shadow_sample": round(extra_ms * 1e6 / max(st["shadow_samples_marched"], 1), 4),
           "same_bits_as_first": None if first is None else bool((first.view(np.uint32) == fb.view(np.uint32)).all())}
    return row, fb


def run_fog_shadows(n, split, steps, warmup, rate, kind, vol, dtype="f32", first=None, bias=1):
    """--fused --shade's lit frame (one light, gvt_hip_volume_frame_fused_shaded) against the same frame with the fog shadowed from the
    baked light grids (gvt_hip_volume_frame_fog_shadowed), alternating frame by frame on one tracer; the bake timed on its own (the
    launch's event time: a cost per change of data, table, surfaces or lights, not per frame); and, as a yardstick, the loop's lit frame
    with the CELL and with the CENTRAL gradient on a second tracer of the same bricks.  Returns (row, the fog-shadowed framebuffer)."""
    bricks = vol if split == (1, 1, 1) else scenes.split_volume(vol, *split, ghosts=True)
    tr = VolumeTracer(bricks, camera(), transfer(kind, dtype), sampling_rate=rate, native=dtype != "f32", fused=True, fused_shaded=True, shadows=True, fog_shadows=True,
                      fog_bias=bias)
    tr.set_lights(SHADE_LIGHTS[:1]).set_shading(True)
    bake = []
    for i in range(warmup + steps):
        tr.rebake()
        bake.append(tr.light_grid_stats["ms"])
    bake = bake[warmup:]
    g = tr.light_grid_stats
    plain, fog = [], []

    def frame(flag):
        tr.shadows = tr.fog_shadows = flag
        tr.frame()

    for i in range(warmup + steps):
        plain.append(timed(lambda: frame(False)))
        ps = tr.stats()
        fog.append(timed(lambda: frame(True)))
    plain, fog = plain[warmup:], fog[warmup:]
    st = tr.stats()
    fb = tr.framebuffer(False).copy()
    ref = VolumeTracer(bricks, camera(), transfer(kind, dtype), sampling_rate=rate, native=dtype != "f32").set_lights(SHADE_LIGHTS[:1]).set_shading(True)
    grad = {"cell": [], "central": []}
    for i in range(warmup + steps):
        for k in grad:
            ref.set_gradient(k)
            grad[k].append(timed(ref.frame))
    grad = {k: v[warmup:] for k, v in grad.items()}
    row = {"mode": "fused_fog_shadows", "n": n, "dtype": dtype, "tf": kind, "bricks": int(np.prod(split)), "sampling_rate": rate, "bias": bias,
           "bake_ms_median": med(bake), "bake_ms_min": round(min(bake), 3), "bake_ms_max": round(max(bake), 3), "bake_rays": int(g["rays"]),
           "bake_mrays_per_s": round(g["rays"] / float(np.median(bake)) / 1e3, 1), "bake_samples": int(g["samples_marched"]),
           "bake_samples_interpolated": int(g["samples_gathered"]), "grid_bytes": int(g["bytes"]), "light_bakes": int(st["light_bakes"]),
           "plain_ms_median": med(plain), "plain_ms_min": round(min(plain), 3), "plain_ms_max": round(max(plain), 3),
           "fog_ms_median": med(fog), "fog_ms_min": round(min(fog), 3), "fog_ms_max": round(max(fog), 3),
           "fog_over_plain": round(float(np.median(fog)) / float(np.median(plain)), 4),
           "samples_per_frame": int(st["samples_marched"]), "samples_interpolated": int(st["samples_gathered"]), "samples_shaded": int(st["samples_shaded"]),
           "fog_samples_shadowed": int(st["fog_samples_shadowed"]),
           "camera_counters_same": bool(all(st[k] == ps[k] for k in ("samples_marched", "samples_gathered", "samples_shaded", "brick_visits", "rays_deposited"))),
           "loop_cell_ms_median": med(grad["cell"]), "loop_central_ms_median": med(grad["central"]),
           "central_over_cell": round(float(np.median(grad["central"])) / float(np.median(grad["cell"])), 4),
           "same_bits_as_first": None if first is None else bool((first.view(np.uint32) == fb.view(np.uint32)).all())}
    return row, fb


def run_mesh_shadows(n, split, steps, warmup, rate, kind, vol, shape, dtype="f32", first=None):
    """The bunny inside the grid: the fog-shadowed frame (shape "surf": surfaces with unlit fog, which is the shadowed frame) against the
    same frame with the meshes' shadows (gvt_hip_volume_frame_mesh_shadowed), alternating frame by frame on one tracer
    (VolumeTracer.mesh_shadows switches the entry point); the occluder bake timed on its own (its launches' event time: a cost per change
    of the scene or the lights, not per frame) and once more under the any-hit profile, for the share of it spent in traversal.  The
    volume is rendered alone and unclipped, so that the two frames march the same samples.  Returns (row, the mesh-shadowed framebuffer)."""
    scene = scenes.bunny_scene(1920, 1080)
    placed = scenes.mesh_in_volume(scene, vol, fill=0.6)
    bricks = placed if split == (1, 1, 1) else scenes.split_volume(placed, *split)
    tr = VolumeTracer(bricks, scene.camera, transfer(kind, dtype), sampling_rate=rate, native=dtype != "f32", fused=True, fused_shaded=True, shadows=True, fog_shadows=True,
                      mesh_shadows=True)
    _, lo, hi = DTYPES[dtype]
    if shape != "lit":
        tr.set_surfaces(tuple(lo + v * (hi - lo) for v in SURFACE_MODES["reached"]), (), 0.3)
    tr.set_lights(SHADE_LIGHTS[:1]).set_shading(shape != "surf")
    bake = []
    for i in range(warmup + steps):
        tr.bake_occluders(scene)
        bake.append(tr.occluder_stats["ms"])
    bake = bake[warmup:]
    g = tr.occluder_stats
    capi.profile(4)  # (the any-hit launches alone)
    capi.stats(reset=True)
    tr.bake_occluders(scene)
    any_ms = float(capi.stats()["ms_any"])
    capi.profile(0)
    fog, mesh = [], []

    def frame(flag):
        tr.mesh_shadows = flag
        tr.frame()

    for i in range(warmup + steps):
        fog.append(timed(lambda: frame(False)))
        ps = tr.stats()
        mesh.append(timed(lambda: frame(True)))
    fog, mesh = fog[warmup:], mesh[warmup:]
    st = tr.stats()
    fb = tr.framebuffer(False).copy()
    row = {"mode": "fused_mesh_shadows", "shape": shape, "n": n, "dtype": dtype, "tf": kind, "bricks": int(np.prod(split)), "sampling_rate": rate, "mesh": "bunny",
           "bake_ms_median": med(bake), "bake_ms_min": round(min(bake), 3), "bake_ms_max": round(max(bake), 3), "bake_rays": int(g["rays"]),
           "bake_rays_blocked": int(g["rays_blocked"]), "bake_any_hit_launches": int(g["any_hit_launches"]), "bake_any_hit_ms": round(any_ms, 3),
           "bake_any_hit_share": round(any_ms / max(float(tr.occluder_stats["ms"]), 1e-9), 3), "grid_bytes": int(g["bytes"]),
           "fog_ms_median": med(fog), "fog_ms_min": round(min(fog), 3), "fog_ms_max": round(max(fog), 3),
           "mesh_ms_median": med(mesh), "mesh_ms_min": round(min(mesh), 3), "mesh_ms_max": round(max(mesh), 3),
           "mesh_over_fog": round(float(np.median(mesh)) / float(np.median(fog)), 4), "mesh_shadowed": int(st["mesh_shadowed"]),
           "samples_per_frame": int(st["samples_marched"]), "samples_interpolated": int(st["samples_gathered"]), "samples_shaded": int(st["samples_shaded"]),
           "crossings_per_frame": int(st["crossings_rendered"]), "shadow_rays": int(st["shadow_rays"]),
           "counters_same": bool(all(st[k] == ps[k] for k in ("samples_marched", "samples_gathered", "samples_shaded", "brick_visits", "rays_deposited", "shadow_rays",
                                                              "shadow_samples_marched"))),
           "same_bits_as_first": None if first is None else bool((first.view(np.uint32) == fb.view(np.uint32)).all())}
    return row, fb


def run_ao(n, split, steps, warmup, rate, kind, vol, shape, dtype="f32", first=None, mesh=False, central=False, dirs=16):
    """Ambient occlusion: the base frame (fog-shadowed; mesh: mesh-shadowed, the bunny inside the grid) against the AO frame
    (gvt_hip_volume_frame_ao), alternating frame by frame on one tracer (VolumeTracer.ao switches the entry point); the AO bake (`dirs`
    Fibonacci directions, 16 lattice steps) timed on its own beside the light grids' bake on the same bricks in the same run -- both a
    cost per change, not per frame.  shape: "lit" or "surf_lit".  central: CENTRAL bricks under the flag.  Returns (row, the AO framebuffer)."""
    scene = scenes.bunny_scene(1920, 1080) if mesh else None
    placed = scenes.mesh_in_volume(scene, vol, fill=0.6) if mesh else vol
    bricks = placed if split == (1, 1, 1) and not central else scenes.split_volume(placed, *split, ghosts=True)
    tr = VolumeTracer(bricks, scene.camera if mesh else camera(), transfer(kind, dtype), sampling_rate=rate, native=dtype != "f32", fused=True, fused_shaded=True,
                      shadows=True, fog_shadows=True, mesh_shadows=mesh, fused_central=central, ao=True, ao_dirs=dirs)
    _, lo, hi = DTYPES[dtype]
    if shape != "lit":
        tr.set_surfaces(tuple(lo + v * (hi - lo) for v in SURFACE_MODES["reached"]), (), 0.3)
    tr.set_lights(SHADE_LIGHTS[:1]).set_shading(True)
    if central:
        tr.set_gradient("central")
    if mesh:
        tr.bake_occluders(scene)
    bake, light = [], []
    for i in range(warmup + steps):
        tr.rebake_ao()
        bake.append(tr.ao_stats["ms"])
        tr.rebake()
        light.append(tr.light_grid_stats["ms"])
    bake, light = bake[warmup:], light[warmup:]
    g = tr.ao_stats
    base, ao = [], []

    def frame(flag):
        tr.ao = flag
        tr.frame()

    for i in range(warmup + steps):
        base.append(timed(lambda: frame(False)))
        ps = tr.stats()
        ao.append(timed(lambda: frame(True)))
    base, ao = base[warmup:], ao[warmup:]
    st = tr.stats()
    fb = tr.framebuffer(False).copy()
    row = {"mode": "fused_ao", "shape": shape, "base": "mesh_shadowed" if mesh else "fog_shadowed", "gradient": "central" if central else "cell", "n": n, "dtype": dtype,
           "tf": kind, "bricks": int(np.prod(split)), "sampling_rate": rate, "ao_dirs": int(dirs), "ao_radius_steps": 16,
           "bake_ms_median": med(bake), "bake_ms_min": round(min(bake), 3), "bake_ms_max": round(max(bake), 3), "bake_rays": int(g["rays"]),
           "bake_mrays_per_s": round(g["rays"] / float(np.median(bake)) / 1e3, 1), "bake_samples": int(g["samples_marched"]),
           "bake_samples_interpolated": int(g["samples_gathered"]), "grid_bytes": int(g["bytes"]), "light_bake_ms_median": med(light),
           "bake_over_light_bake": round(float(np.median(bake)) / float(np.median(light)), 3),
           "base_ms_median": med(base), "base_ms_min": round(min(base), 3), "base_ms_max": round(max(base), 3),
           "ao_ms_median": med(ao), "ao_ms_min": round(min(ao), 3), "ao_ms_max": round(max(ao), 3),
           "ao_over_base": round(float(np.median(ao)) / float(np.median(base)), 4), "ao": int(st["ao"]),
           "samples_per_frame": int(st["samples_marched"]), "samples_interpolated": int(st["samples_gathered"]), "samples_shaded": int(st["samples_shaded"]),
           "crossings_per_frame": int(st["crossings_rendered"]), "shadow_rays": int(st["shadow_rays"]),
           "counters_same": bool(all(st[k] == ps[k] for k in ("samples_marched", "samples_gathered", "samples_shaded", "brick_visits", "rays_deposited", "shadow_rays",
                                                              "shadow_samples_marched"))),
           "same_bits_as_first": None if first is None else bool((first.view(np.uint32) == fb.view(np.uint32)).all())}
    return row, fb


def run_shade(n, split, steps, warmup, rate, kind, vol, dtype="f32"):
    """The frame unlit, with one light and with three, alternating on one tracer (the same rays and samples: what the lighting costs)."""
    bricks = vol if split == (1, 1, 1) else scenes.split_volume(vol, *split)
    tr = VolumeTracer(bricks, camera(), transfer(kind, dtype), sampling_rate=rate, native=dtype != "f32")
    modes = {"unlit": 0, "lit1": 1, "lit3": 3}
    ms = {k: [] for k in modes}
    shaded = {}
    for i in range(warmup + steps):
        for k, n_lights in modes.items():
            tr.set_lights(SHADE_LIGHTS[:n_lights]).set_shading(n_lights > 0)
            s0 = tr.stats()["samples_shaded"] if i == warmup else 0
            ms[k].append(timed(tr.frame))
            if i == warmup:
                shaded[k] = tr.stats()["samples_shaded"] - s0
    st = tr.stats()
    out = {"mode": "shade", "n": n, "dtype": dtype, "tf": kind, "bricks": int(np.prod(split)),
           "samples_per_frame": int(st["samples_marched"] / (3 * (warmup + steps))), "samples_interpolated": int(st["samples_gathered"] / (3 * (warmup + steps)))}
    for k in modes:
        v = ms[k][warmup:]
        out.update({k + "_ms_median": med(v), k + "_ms_min": round(min(v), 3), k + "_ms_max": round(max(v), 3), k + "_samples_shaded": int(shaded[k])})
    for k in ("lit1", "lit3"):
        out[k + "_over_unlit"] = round(out[k + "_ms_median"] / out["unlit_ms_median"], 4)
    return out


SMOOTH_ISO = [0.45, 0.55]
CENTRAL_FRAMES = ("shadows", "fog_shadows", "mesh_shadows")


def run_fused_central(n, split, steps, warmup, rate, kind, vol, what, dtype="f32"):
    """--shade --gradient central's lit frame (what = "lit": three lights) or isosurface frame ("iso": two isovalues, shading off) with the
    CENTRAL gradient on every brick: the loop against the fused frame (GVT_HIP_FUSED_CENTRAL), alternating frame by frame on one tracer
    whose bricks carry their ghost faces; the framebuffers compared after every pair."""
    bricks = scenes.split_volume(vol, *split, ghosts=True)
    tr = VolumeTracer(bricks, camera(), transfer(kind, dtype), sampling_rate=rate, native=dtype != "f32", fused=True, fused_shaded=True, fused_central=True)
    _, lo, hi = DTYPES[dtype]
    tr.set_lights(SHADE_LIGHTS)
    if what == "iso":
        tr.set_surfaces([lo + v * (hi - lo) for v in SMOOTH_ISO], (), 0.5).set_shading(False)
    else:
        tr.set_shading(True)
    tr.set_gradient("central")
    loop, fused = [], []
    same = True

    def frame(flag):
        tr.fused = flag
        tr.frame()

    for i in range(warmup + steps):
        loop.append(timed(lambda: frame(False)))
        loop_calls = tr.calls
        a = tr.framebuffer(False).copy()
        fused.append(timed(lambda: frame(True)))
        same = same and bool((a.view(np.uint32) == tr.framebuffer(False).view(np.uint32)).all())  # (outside the timed region)
    loop, fused = loop[warmup:], fused[warmup:]
    st = tr.stats()
    return {"mode": "fused_central_" + what, "n": n, "dtype": dtype, "tf": kind, "bricks": int(np.prod(split)), "sampling_rate": rate, "features": int(st["features"]),
            "fused": int(st["fused"]), "loop_ms_median": med(loop), "loop_ms_min": round(min(loop), 3), "loop_ms_max": round(max(loop), 3), "loop_adapter_calls": int(loop_calls),
            "fused_ms_median": med(fused), "fused_ms_min": round(min(fused), 3), "fused_ms_max": round(max(fused), 3),
            "samples_per_frame": int(st["samples_marched"]), "samples_interpolated": int(st["samples_gathered"]), "samples_shaded": int(st["samples_shaded"]),
            "crossings_per_frame": int(st["crossings_rendered"]), "brick_visits": int(st["brick_visits"]),
            "fused_over_loop": round(float(np.median(fused)) / float(np.median(loop)), 4), "fused_wins": bool(max(fused) < min(loop)), "same_bits": same}


def run_central_shadows(n, split, steps, warmup, rate, kind, vol, which, dtype="f32", first=None):
    """A shadowed frame (which: one of CENTRAL_FRAMES) of two isovalues in lit fog under one light, with the CELL and with the CENTRAL
    gradient (GVT_HIP_VOLUME_ALLOW_CENTRAL), alternating frame by frame on one tracer whose bricks carry their ghost faces: what the
    smooth gradient costs inside the shadowed kernels.  The grids are baked once -- the kind makes none stale.  mesh_shadows: the bunny
    inside the grid, as --mesh-shadows has it.  first: the CENTRAL framebuffer of another bricking, compared bitwise."""
    cam = camera()
    scene = None
    if which == "mesh_shadows":
        scene = scenes.bunny_scene(1920, 1080)
        vol, cam = scenes.mesh_in_volume(scene, vol, fill=0.6), scene.camera
    bricks = scenes.split_volume(vol, *split, ghosts=True)
    tr = VolumeTracer(bricks, cam, transfer(kind, dtype), sampling_rate=rate, native=dtype != "f32", fused=True, fused_shaded=True, shadows=True,
                      fog_shadows=which != "shadows", mesh_shadows=which == "mesh_shadows", fused_central=True)
    _, lo, hi = DTYPES[dtype]
    tr.set_surfaces([lo + v * (hi - lo) for v in SMOOTH_ISO], (), 0.5).set_lights(SHADE_LIGHTS[:1]).set_shading(True)
    if scene is not None:
        tr.bake_occluders(scene)
    ms = {"cell": [], "central": []}
    stats, fbs = {}, {}
    for i in range(warmup + steps):
        for g in ms:
            tr.set_gradient(g)
            ms[g].append(timed(tr.frame))
            if i == warmup + steps - 1:
                stats[g], fbs[g] = tr.stats(), tr.framebuffer(False).copy()
    ms = {g: v[warmup:] for g, v in ms.items()}
    st, sc_ = stats["central"], stats["cell"]
    keys = ("samples_marched", "samples_gathered", "samples_shaded", "crossings_rendered", "brick_visits", "rays_deposited", "shadow_rays", "shadow_brick_visits",
            "shadow_crossings", "shadow_samples_marched", "shadow_samples_gathered")
    row = {"mode": "central_" + which, "n": n, "dtype": dtype, "tf": kind, "bricks": int(np.prod(split)), "sampling_rate": rate, "features": int(st["features"]),
           "cell_features": int(sc_["features"]), "shadowed": int(st["shadowed"]), "light_bakes": int(st.get("light_bakes", 0)), "occluder_bakes": int(st.get("occluder_bakes", 0))}
    for g, v in ms.items():
        row.update({g + "_ms_median": med(v), g + "_ms_min": round(min(v), 3), g + "_ms_max": round(max(v), 3)})
    row.update({"central_over_cell": round(float(np.median(ms["central"])) / float(np.median(ms["cell"])), 4),
                "samples_per_frame": int(st["samples_marched"]), "samples_shaded": int(st["samples_shaded"]), "crossings_per_frame": int(st["crossings_rendered"]),
                "shadow_rays": int(st["shadow_rays"]), "shadow_samples": int(st["shadow_samples_marched"]),
                "counters_same": bool(all(st[k] == sc_[k] for k in keys)),
                "alpha_same": bool((fbs["cell"][..., 3].view(np.uint32) == fbs["central"][..., 3].view(np.uint32)).all()),
                "colour_differs": bool((fbs["cell"][..., :3].view(np.uint32) != fbs["central"][..., :3].view(np.uint32)).any()),
                "same_bits_as_first": None if first is None else bool((first.view(np.uint32) == fbs["central"].view(np.uint32)).all())})
    return row, fbs["central"]


def run_smooth(n, split, steps, warmup, rate, kind, vol, dtype="f32"):
    """The lit frame (three lights) and the isosurface frame (two isovalues, lights, shading off), each with the CELL and with the
    CENTRAL gradient, alternating on one tracer whose bricks carry their ghost faces: what central differences cost."""
    bricks = vol if split == (1, 1, 1) else scenes.split_volume(vol, *split, ghosts=True)
    tr = VolumeTracer(bricks, camera(), transfer(kind, dtype), sampling_rate=rate, native=dtype != "f32").set_lights(SHADE_LIGHTS)
    _, lo, hi = DTYPES[dtype]
    frames = {"lit": lambda: tr.set_surfaces().set_shading(True), "iso": lambda: tr.set_surfaces([lo + v * (hi - lo) for v in SMOOTH_ISO], (), 0.5).set_shading(False)}
    ms = {(f, g): [] for f in frames for g in ("cell", "central")}
    count = {}
    for i in range(warmup + steps):
        for f, setup in frames.items():
            setup()
            for g in ("cell", "central"):
                tr.set_gradient(g)
                s0 = tr.stats() if i == warmup else None
                ms[f, g].append(timed(tr.frame))
                if i == warmup:
                    s1 = tr.stats()
                    count[f, g] = (s1["samples_shaded"] - s0["samples_shaded"], s1["crossings_rendered"] - s0["crossings_rendered"])
    out = {"mode": "smooth", "n": n, "dtype": dtype, "tf": kind, "bricks": int(np.prod(split)), "central_marches": tr.stats()["central_marches"]}
    for (f, g), v in ms.items():
        v = v[warmup:]
        out.update({"%s_%s_ms_median" % (f, g): med(v), "%s_%s_ms_min" % (f, g): round(min(v), 3), "%s_%s_ms_max" % (f, g): round(max(v), 3),
                    "%s_%s_samples_shaded" % (f, g): int(count[f, g][0]), "%s_%s_crossings" % (f, g): int(count[f, g][1])})
    for f in frames:
        out[f + "_central_over_cell"] = round(out[f + "_central_ms_median"] / out[f + "_cell_ms_median"], 4)
    return out


def run_mixed(n, split, steps, warmup, rate, vol, dtype="f32"):
    """bun_zipper inside the grid at 1080p: the mixed frame and its four parts, each ended by a synchronisation."""
    from gravit_amd.scheduler import MixedTracer

    scene = scenes.bunny70k_scene(1920, 1080)
    placed = scenes.mesh_in_volume(scene, vol, fill=0.6)
    bricks = placed if split == (1, 1, 1) else scenes.split_volume(placed, *split)
    mt = MixedTracer(scene, bricks, scene.camera, transfer("thin", dtype), sampling_rate=rate, native=dtype != "f32")
    parts = {"frame": [], "mesh": [], "depth": [], "volume": [], "volume_unclipped": [], "composite": []}
    B = mt.mesh.backend
    for i in range(warmup + steps):
        parts["frame"].append(timed(mt.frame))
        parts["mesh"].append(timed(mt.mesh))
        parts["depth"].append(timed(lambda: mt.depth.render(B, mt.camera)))
        parts["volume"].append(timed(lambda: mt.volume.frame(mt.depth)))
        parts["composite"].append(timed(lambda: mt.volume.fb.composite_over(B.fb, mt.depth)))
        parts["volume_unclipped"].append(timed(mt.volume.frame))
    fb = mt.frame().framebuffer(False)
    depth = mt.depth.download()
    out = {"mode": "mixed", "n": n, "dtype": dtype, "bricks": int(np.prod(split)), "mesh": "bun_zipper", "wall_pixels": int(np.isfinite(depth).sum()),
           "lit_pixels": int((fb[..., 3] > 0).sum())}
    for k, v in parts.items():
        out[k + "_ms_median"] = med(v[warmup:])
        out[k + "_ms_min"] = round(min(v[warmup:]), 3)
    return out


def run_amr(n, steps, warmup, rate):
    """Configurations (a)-(d) alternating on four tracers, then (e) on its own; one line per configuration."""
    base = noise(n, "f32")
    cells = n - 1
    lo, ext = cells // 4, cells // 2  # the central eighth, in cells
    vols = {"a_plain": base, "b_empty_set": scenes.VolumeData(base.data, base.origin, base.spacing)}
    c = scenes.VolumeData(base.data, base.origin, base.spacing)
    s0 = scenes.refine(c, (lo,) * 3, (ext,) * 3, 2, seed=1)
    d = scenes.VolumeData(base.data, base.origin, base.spacing, list(c.subgrids))
    scenes.refine(d, (ext // 2,) * 3, (ext,) * 3, 4, parent=s0, seed=2)  # (the subgrid has 2 * ext cells per axis)
    vols["c_ratio2"], vols["d_ratio2_ratio4"] = c, d
    cam, t = camera(), transfer("thin")
    trs = {k: VolumeTracer(v, cam, t, sampling_rate=rate) for k, v in vols.items()}
    trs["b_empty_set"].adapters[0].set_subgrids([])
    ms = {k: [] for k in trs}
    first = {}
    for i in range(warmup + steps):
        for k, tr in trs.items():
            if i == warmup:
                first[k] = tr.stats()
            ms[k].append(timed(tr.frame))
    out = []
    for k, tr in trs.items():
        st, amr, v = tr.stats(), tr.adapters[0].amr_info(), ms[k][warmup:]
        out.append({"mode": "amr", "config": k, "n": n, "sampling_rate": rate, "ms_median": med(v), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
                    "samples_per_frame": int((st["samples_marched"] - first[k]["samples_marched"]) / steps),
                    "samples_refined_per_frame": int((st["samples_refined"] - first[k]["samples_refined"]) / steps),
                    "amr_marches_per_frame": (st["amr_marches"] - first[k]["amr_marches"]) / steps, "n_subgrids": amr["n_subgrids"], "n_levels": amr["n_levels"],
                    "device_mb": round((4.0 * n ** 3 + amr["subgrid_bytes"]) / 1e6, 1), "lit_pixels": int((tr.framebuffer(False)[..., 3] > 0).sum())})
    for r in out:
        r["vs_plain"] = round(r["ms_median"] / out[0]["ms_median"], 4)
    for tr in trs.values():
        for a in tr.adapters:
            a.close()
    del trs, vols, c, d
    big = noise(2 * n, "f32")  # (e): the whole domain at the subgrid's resolution
    big.spacing = np.full(3, F(1.0 / (2 * n - 1)), F)
    tr = VolumeTracer(big, cam, t, sampling_rate=rate)
    v = [timed(tr.frame) for _ in range(warmup + steps)][warmup:]
    st = tr.stats()
    out.append({"mode": "amr", "config": "e_uniform_2n", "n": 2 * n, "sampling_rate": rate, "ms_median": med(v), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
                "samples_per_frame": int(st["samples_marched"] / (warmup + steps)), "samples_refined_per_frame": 0, "amr_marches_per_frame": 0.0, "n_subgrids": 0,
                "n_levels": 1, "device_mb": round(4.0 * (2 * n) ** 3 / 1e6, 1), "lit_pixels": int((tr.framebuffer(False)[..., 3] > 0).sum()),
                "vs_plain": round(med(v) / out[0]["ms_median"], 4)})
    return out


def run_amr_shaded(n, steps, warmup, rate, what):
    """--amr --surfaces / --amr --shade: run_amr's grid, subgrids (ratio 2 with its ratio-4 child), table and rate.  Three tracers alternate
    frame by frame: the flagged AMR volume under the surfaces (what == "surfaces": the "reached" isovalues, opacity 0.3, one light) or
    the lit shading (what == "shade": one light); the same level-0 volume without subgrids under the same surfaces / shading; and the
    plain AMR frame.  One line."""
    base = noise(n, "f32")
    cells = n - 1
    lo, ext = cells // 4, cells // 2
    d = scenes.VolumeData(base.data, base.origin, base.spacing)
    s0 = scenes.refine(d, (lo,) * 3, (ext,) * 3, 2, seed=1)
    scenes.refine(d, (ext // 2,) * 3, (ext,) * 3, 4, parent=s0, seed=2)
    cam, t = camera(), transfer("thin")
    trs = {"amr_shaded": VolumeTracer(d, cam, t, sampling_rate=rate, amr_shaded=True), "plain_shaded": VolumeTracer(base, cam, t, sampling_rate=rate),
           "amr_fog": VolumeTracer(d, cam, t, sampling_rate=rate)}
    for k in ("amr_shaded", "plain_shaded"):
        if what == "surfaces":
            trs[k].set_surfaces(SURFACE_MODES["reached"], (), 0.3).set_lights([((3.0, 4.0, 5.0), (1.0, 1.0, 1.0))])
        else:
            trs[k].set_lights(SHADE_LIGHTS[:1]).set_shading(True)
    ms = {k: [] for k in trs}
    first = {}
    for i in range(warmup + steps):
        for k, tr in trs.items():
            if i == warmup:
                first[k] = tr.stats()
            ms[k].append(timed(tr.frame))
    out = {"mode": "amr_" + what, "n": n, "sampling_rate": rate, "n_subgrids": 2, "n_levels": 3}
    for k, tr in trs.items():
        st, v = tr.stats(), ms[k][warmup:]
        out.update({k + "_ms_median": med(v), k + "_ms_min": round(min(v), 3), k + "_ms_max": round(max(v), 3),
                    k + "_samples_per_frame": int((st["samples_marched"] - first[k]["samples_marched"]) / steps),
                    k + "_samples_refined_per_frame": int((st["samples_refined"] - first[k]["samples_refined"]) / steps),
                    k + "_crossings_per_frame": int((st["crossings_rendered"] - first[k]["crossings_rendered"]) / steps),
                    k + "_samples_shaded_per_frame": int((st["samples_shaded"] - first[k]["samples_shaded"]) / steps),
                    k + "_amr_marches_per_frame": (st["amr_marches"] - first[k]["amr_marches"]) / steps,
                    k + "_lit_pixels": int((tr.framebuffer(False)[..., 3] > 0).sum())})
    out["amr_shaded_over_plain_shaded"] = round(out["amr_shaded_ms_median"] / out["plain_shaded_ms_median"], 4)
    out["amr_shaded_over_amr_fog"] = round(out["amr_shaded_ms_median"] / out["amr_fog_ms_median"], 4)
    return out


def amr_bricked_scene(n):
    """--fused --amr: the noise grid with its central eighth refined at ratio 2, given as EIGHT level-1 subgrids cut along the faces of
    the 4 x 4 x 4 bricking (split_volume's even cuts), so that each lies in one brick of every bricking measured (1, 8 and 64); a ratio-4
    child over the central cells of two of them (the first and the last)."""
    vol = noise(n, "f32")
    cells = n - 1
    lo, hi = cells // 4, cells // 4 + cells // 2  # the central eighth, in cells: run_amr's
    faces = [c for c in scenes._cuts(n, 4) if lo < c < hi]
    edges = [lo] + faces + [hi]
    boxes = [(a0, a1) for a0, a1 in zip(edges, edges[1:])]
    level1 = []
    for z0, z1 in boxes:
        for y0, y1 in boxes:
            for x0, x1 in boxes:
                level1.append(scenes.refine(vol, (x0, y0, z0), (x1 - x0, y1 - y0, z1 - z0), 2, seed=1 + len(level1)))
    for s in (level1[0], level1[-1]):
        c = np.asarray(vol.subgrids[s].cells) * 2  # the subgrid's own cells per axis
        scenes.refine(vol, tuple(int(v) // 4 for v in c), tuple(int(v) // 2 for v in c), 4, parent=s, seed=100 + s)
    return vol


def run_fused_amr(n, split, steps, warmup, rate, vol, shaded=None):
    """--fused --amr [--surfaces] [--shade]: amr_bricked_scene in the bricking `split` under the "thin" table.  Three tracers alternate
    frame by frame in one process: the loop over the AMR bricks, the fused AMR frame (gvt_hip_volume_frame_fused_amr) over the same
    bricks, and the fused frame over the same level-0 grid without subgrids.  shaded: None (fog), "surfaces" (the "reached" isovalues,
    opacity 0.3, one light) or "lit" (lit fog by one light).  The loop's and the fused AMR framebuffer are compared in every bit once."""
    cam, t = camera(), transfer("thin")
    plain = scenes.VolumeData(vol.data, vol.origin, vol.spacing)
    bricks = vol if split == (1, 1, 1) else scenes.split_amr_volume(vol, *split)
    bare = plain if split == (1, 1, 1) else scenes.split_volume(plain, *split)
    trs = {"loop": VolumeTracer(bricks, cam, t, sampling_rate=rate, amr_shaded=True),
           "fused": VolumeTracer(bricks, cam, t, sampling_rate=rate, amr_shaded=True, fused=True, fused_shaded=True, fused_amr=True),
           "plain_fused": VolumeTracer(bare, cam, t, sampling_rate=rate, fused=True, fused_shaded=True)}
    for tr in trs.values():
        if shaded == "surfaces":
            tr.set_surfaces(SURFACE_MODES["reached"], (), 0.3).set_lights([((3.0, 4.0, 5.0), (1.0, 1.0, 1.0))])
        elif shaded == "lit":
            tr.set_lights(SHADE_LIGHTS[:1]).set_shading(True)
    ms = {k: [] for k in trs}
    for i in range(warmup + steps):
        for k, tr in trs.items():
            ms[k].append(timed(tr.frame))
    ms = {k: v[warmup:] for k, v in ms.items()}
    same = bool((trs["loop"].framebuffer(False).view(np.uint32) == trs["fused"].framebuffer(False).view(np.uint32)).all())
    st, pst = trs["fused"].stats(), trs["plain_fused"].stats()
    out = {"mode": "fused_amr" if not shaded else "fused_amr_" + shaded, "n": n, "bricks": int(np.prod(split)), "sampling_rate": rate, "n_subgrids": len(vol.subgrids),
           "loop_adapter_calls": int(trs["loop"].calls)}
    for k, v in ms.items():
        out.update({k + "_ms_median": med(v), k + "_ms_min": round(min(v), 3), k + "_ms_max": round(max(v), 3)})
    out.update({"fused": int(st["fused"]), "features": int(st["features"]), "amr_bricks": int(st["amr_bricks"]), "brick_visits": int(st["brick_visits"]),
                "samples_per_frame": int(st["samples_marched"]), "samples_interpolated": int(st["samples_gathered"]), "samples_refined": int(st["samples_refined"]),
                "crossings_per_frame": int(st["crossings_rendered"]), "samples_shaded": int(st["samples_shaded"]),
                "plain_fused_features": int(pst["features"]), "plain_fused_samples_per_frame": int(pst["samples_marched"]),
                "fused_over_loop": round(float(np.median(ms["fused"])) / float(np.median(ms["loop"])), 4),
                "fused_over_plain_fused": round(float(np.median(ms["fused"])) / float(np.median(ms["plain_fused"])), 4),
                "fused_median_below_loop_min": bool(float(np.median(ms["fused"])) < min(ms["loop"])), "same_bits": same,
                "lit_pixels": int((trs["fused"].framebuffer(False)[..., 3] > 0).sum())})
    for tr in trs.values():
        for a in tr.adapters:
            a.close()
    return out


def run_shadow_amr(n, split, steps, warmup, rate, vol, frame, shape, first=None):
    """--fused --amr with --shadows / --fog-shadows / --mesh-shadows: amr_bricked_scene in the bricking `split` under the "thin" table.
    frame: "shadowed", "fog" or "mesh"; shape: "surf" (the "reached" isovalues, opacity 0.3, unlit fog), "lit" (lit fog alone: the lean
    kernels) or "surf_lit"; one light.  Two tracers alternate frame by frame: the frame over the AMR bricks (shadow_amr=True) and the
    same frame over the same level-0 grid without subgrids -- there is no loop to compare with.  The bakes of both are timed on their own
    (the launches' event time).  first: the AMR framebuffer of another bricking, compared bitwise.  Returns (row, the AMR framebuffer)."""
    t = transfer("thin")
    scene = scenes.bunny_scene(1920, 1080) if frame == "mesh" else None
    cam = scene.camera if scene is not None else camera()
    if scene is not None:  # the bunny inside the grid: the subgrids are index boxes, they move with it
        placed = scenes.mesh_in_volume(scene, vol, fill=0.6)
        vol = scenes.VolumeData(placed.data, placed.origin, placed.spacing, vol.subgrids)
    plain = scenes.VolumeData(vol.data, vol.origin, vol.spacing)
    bricks = vol if split == (1, 1, 1) else scenes.split_amr_volume(vol, *split)
    bare = plain if split == (1, 1, 1) else scenes.split_volume(plain, *split)
    how = dict(sampling_rate=rate, shadows=True, fog_shadows=frame != "shadowed", mesh_shadows=frame == "mesh")
    trs = {"amr": VolumeTracer(bricks, cam, t, amr_shaded=True, shadow_amr=True, **how), "plain": VolumeTracer(bare, cam, t, **how)}
    for tr in trs.values():
        if shape != "lit":
            tr.set_surfaces(SURFACE_MODES["reached"], (), 0.3)
        tr.set_lights(SHADE_LIGHTS[:1]).set_shading(shape != "surf")
    bakes = {}
    for k, tr in trs.items():
        if frame != "shadowed" and shape != "surf":
            bakes[k + "_light_bake"] = []
            for i in range(warmup + steps):
                tr.rebake()
                bakes[k + "_light_bake"].append(tr.light_grid_stats["ms"])
        if frame == "mesh":
            bakes[k + "_occluder_bake"] = []
            for i in range(warmup + steps):
                tr.bake_occluders(scene)
                bakes[k + "_occluder_bake"].append(tr.occluder_stats["ms"])
    ms = {k: [] for k in trs}
    for i in range(warmup + steps):
        for k, tr in trs.items():
            ms[k].append(timed(tr.frame))
    ms = {k: v[warmup:] for k, v in ms.items()}
    st, pst = trs["amr"].stats(), trs["plain"].stats()
    fb = trs["amr"].framebuffer(False).copy()
    out = {"mode": "shadow_amr_" + frame, "shape": shape, "n": n, "bricks": int(np.prod(split)), "sampling_rate": rate, "n_subgrids": len(vol.subgrids)}
    for k, v in list(ms.items()) + [(k, v[warmup:]) for k, v in bakes.items()]:
        out.update({k + "_ms_median": med(v), k + "_ms_min": round(min(v), 3), k + "_ms_max": round(max(v), 3)})
    out["amr_over_plain"] = round(float(np.median(ms["amr"])) / float(np.median(ms["plain"])), 4)
    for b in ("light_bake", "occluder_bake"):
        if "amr_" + b in bakes:
            out[b + "_amr_over_plain"] = round(float(np.median(bakes["amr_" + b][warmup:])) / float(np.median(bakes["plain_" + b][warmup:])), 4)
    out.update({"shadowed": int(st["shadowed"]), "features": int(st["features"]), "plain_features": int(pst["features"]), "brick_visits": int(st["brick_visits"]),
                "samples_per_frame": int(st["samples_marched"]), "samples_interpolated": int(st["samples_gathered"]), "crossings_per_frame": int(st["crossings_rendered"]),
                "samples_shaded": int(st["samples_shaded"]), "shadow_rays": int(st["shadow_rays"]), "shadow_samples": int(st["shadow_samples_marched"]),
                "plain_samples_per_frame": int(pst["samples_marched"]), "plain_shadow_samples": int(pst["shadow_samples_marched"]),
                "lit_pixels": int((fb[..., 3] > 0).sum()),
                "same_bits_as_first": None if first is None else bool((first.view(np.uint32) == fb.view(np.uint32)).all())})
    for tr in trs.values():
        for a in tr.adapters:
            a.close()
    return out, fb


def run_domains(n, split, world, steps, warmup, rate, kind, vol, per_queue, overlap):
    """One bricking at one world size: `world` threads, each a rank with its own HipVolumeBackend, frames started together."""
    import threading

    import torch

    from gravit_amd.scheduler import HipVolumeBackend, VolumeDomainTracer
    from tests.fake_dist import FakeWorld

    class PerQueueBackend(HipVolumeBackend):  # the exchange as HipBackend does it: one export / append call per brick
        def export_wire(self, insts, torch, device):
            sizes = [len(self.queues[i]) for i in insts]
            buf = torch.empty((sum(sizes), 20), dtype=torch.float32, device=device)
            off = 0
            for i, cnt in zip(insts, sizes):
                if cnt:
                    self.queues[i].export_device(buf.data_ptr() + off * 80, cnt)
                    self.queues[i].clear()
                off += cnt
            return buf

        def append_wire(self, insts, buf, off, counts):
            for i, cnt in zip(insts, counts):
                self.queues[i].append_device(buf.data_ptr() + off * 80, cnt)
                off += cnt

    lock = threading.Lock()

    class Timed:  # one thread inside the library at a time; the exchange's own calls are timed inside the lock
        def __init__(self, inner, acc):
            self._b, self._acc = inner, acc

        def __getattr__(self, name):
            attr = getattr(self._b, name)
            if not callable(attr):
                return attr

            def call(*a, **k):
                with lock:
                    if name not in ("export_wire", "append_wire"):
                        return attr(*a, **k)
                    t = time.perf_counter()
                    r = attr(*a, **k)
                    capi.synchronize()
                    self._acc[name] += time.perf_counter() - t
                    return r
            return call

    class TimedDist:  # the payload's way through the transport: posting and waiting
        def __init__(self, inner, acc):
            self._d, self._acc = inner, acc

        def __getattr__(self, name):
            return getattr(self._d, name)

        def batch_isend_irecv(self, ops):
            if any(op.tensor.dim() != 2 for op in ops):  # (the composite's rectangles: not the ray exchange)
                return self._d.batch_isend_irecv(ops)
            t = time.perf_counter()
            for r in self._d.batch_isend_irecv(ops):
                r.wait()  # (a receive also waits for its peer to reach the exchange)
            torch.cuda.current_stream().synchronize()
            self._acc["transfer"] += time.perf_counter() - t
            return []

    bricks = scenes.split_volume(vol, *split)
    owner = [i % world for i in range(len(bricks))]
    cam, tf = camera(), transfer(kind)
    fw = FakeWorld(world)
    start = threading.Barrier(world)
    res, errs = {}, []

    def rank_main(rank):
        try:
            acc = {"export_wire": 0.0, "append_wire": 0.0, "transfer": 0.0}
            with lock:
                B = (PerQueueBackend if per_queue else HipVolumeBackend)(bricks, cam, tf, None, rate, True, False, [o == rank for o in owner])
            tr = VolumeDomainTracer(bricks, owner, cam, tf, TimedDist(fw.rank_view(rank), acc), torch, torch.device("cuda", 0), sampling_rate=rate,
                                    backend=Timed(B, acc), overlap=overlap)
            frames, shares = [], []
            for i in range(warmup + steps):
                for k in acc:
                    acc[k] = 0.0
                start.wait()
                t = time.perf_counter()
                tr()
                tr.composite(download=False)
                with lock:
                    capi.synchronize()
                start.wait()  # (the frame is over when every rank has composited)
                frames.append((time.perf_counter() - t) * 1e3)
                shares.append(dict(acc))
            res[rank] = (frames[warmup:], shares[warmup:], tr.rounds, tr.rays_sent, tr.adapter_calls)
        except Exception:  # noqa: BLE001
            import traceback

            errs.append(traceback.format_exc())
            for b in (fw.barrier, start):
                b.abort()

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=900) for t in th]
    if errs:
        raise RuntimeError(errs[0])
    frames = res[0][0]
    ex = [max(1e3 * sum(res[r][1][i].values()) for r in range(world)) for i in range(steps)]
    parts = {k: med([max(1e3 * res[r][1][i][k] for r in range(world)) for i in range(steps)]) for k in ("export_wire", "transfer", "append_wire")}
    return {"mode": "domains", "n": n, "tf": kind, "bricks": len(bricks), "world": world, "exchange": "per_queue" if per_queue else "batched",
            "loop": "overlapped" if overlap else "bsp", "ms_median": med(frames), "ms_min": round(min(frames), 3), "ms_max": round(max(frames), 3),
            "rounds": res[0][2], "rays_sent": sum(res[r][3] for r in range(world)), "adapter_calls": sum(res[r][4] for r in range(world)),
            "exchange_ms_median": med(ex), "exchange_share": round(float(np.median(ex)) / float(np.median(frames)), 4), "export_ms": parts["export_wire"],
            "transfer_ms": parts["transfer"], "append_ms": parts["append_wire"]}


def run_update(n, device, steps, warmup, recreate_only, dtype="f32"):
    """Two time steps of the n^3 noise grid, pushed alternately into one brick under the sparse table."""
    from gravit_amd.adapter import HipVolumeAdapter

    data = [quantise(scenes.noise_volume(n, seed=s).data, dtype) for s in (1, 2)]
    native, vbytes = dtype != "f32", np.dtype(DTYPES[dtype][0]).itemsize
    geo = (np.zeros(3, F), np.full(3, F(1.0 / (n - 1)), F))
    if device:
        import torch

        data = [torch.from_numpy(d).cuda() for d in data]
        torch.cuda.synchronize()
    t = transfer("spikes", dtype)
    out = {"n": n, "dtype": dtype, "samples": "device" if device else "host", "grid_mb": round(vbytes * n ** 3 / 1e6, 1)}
    ad, wall = None, []
    for i in range(warmup + steps):  # what a new time step cost without the update: a new brick (a tracer around it not counted)
        t0 = time.perf_counter()
        if ad is not None:
            ad.close()
        ad = HipVolumeAdapter(scenes.VolumeData(data[i % 2], *geo), 1.0, native=native)
        ad.set_transfer(t)
        capi.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    out["recreate_wall_ms"], out["recreate_wall_min_ms"] = med(wall[warmup:]), round(min(wall[warmup:]), 3)
    out["n_blocks"], out["n_blocks_empty"] = ad.info()["n_blocks"], ad.info()["n_blocks_empty"]
    if recreate_only:
        return out
    bare = HipVolumeAdapter(scenes.VolumeData(data[0], *geo), 1.0, native=native)  # no transfer function: its update is ranges + download alone
    wall, ms, ms_bare, ms_kernel = [], [], [], []
    for i in range(warmup + steps):  # profiling off: the wall time and both ms_out
        t0 = time.perf_counter()
        ms.append(ad.update_samples(data[(i + 1) % 2]))
        wall.append((time.perf_counter() - t0) * 1e3)
        ms_bare.append(bare.update_samples(data[(i + 1) % 2]))
    capi.profile(1)
    for i in range(warmup + steps):  # a pass of its own for the range kernels' event time (the profiling events are not in the times above)
        k0 = capi.stats()["ms_build"]
        ad.update_samples(data[(i + 1) % 2])
        ms_kernel.append(capi.stats()["ms_build"] - k0)
    capi.profile(0)
    w = warmup
    out.update({"update_wall_ms": med(wall[w:]), "update_wall_min_ms": round(min(wall[w:]), 3), "update_ms_out": med(ms[w:]),
                "range_kernels_ms": med(ms_kernel[w:]), "ranges_and_download_ms": med(ms_bare[w:]),
                "table_rebuild_ms": med(np.array(ms[w:]) - np.array(ms_bare[w:])),
                "range_kernel_gbs_of_grid": round(vbytes * n ** 3 / 1e6 / max(float(np.median(ms_kernel[w:])), 1e-9), 1),
                "recreate_over_update": round(out["recreate_wall_ms"] / max(float(np.median(wall[w:])), 1e-9), 1)})
    return out


def run_amr_update(n, device, steps, warmup, three_call_only):
    """--update --amr: two time steps of amr_bricked_scene(n) (step 2: every sample v of every level becomes 1 - v), pushed alternately into
    one brick under the sparse table."""
    from gravit_amd.adapter import HipVolumeAdapter

    vol = amr_bricked_scene(n)
    level0 = [vol.data, np.ascontiguousarray(F(1.0) - vol.data)]
    subs = [list(vol.subgrids), [scenes.Subgrid(s.parent, s.ratio, s.lo, s.cells, np.ascontiguousarray(F(1.0) - s.data)) for s in vol.subgrids]]
    sub_mb = 4.0 * sum(s.data.size for s in vol.subgrids) / 1e6
    if device:
        import torch

        level0 = [torch.from_numpy(d).cuda() for d in level0]
        subs = [[scenes.Subgrid(s.parent, s.ratio, s.lo, s.cells, torch.from_numpy(s.data).cuda()) for s in step] for step in subs]
        torch.cuda.synchronize()
    t = transfer("spikes", "f32")
    ad = HipVolumeAdapter(vol, 2.0)
    ad.set_transfer(t)
    out = {"mode": "amr_update", "n": n, "samples": "device" if device else "host", "grid_mb": round(4.0 * n ** 3 / 1e6, 1), "subgrid_mb": round(sub_mb, 1),
           "n_subgrids": len(vol.subgrids)}
    wall = []
    for i in range(warmup + steps):  # the documented route before the in-place call
        k = (i + 1) % 2
        t0 = time.perf_counter()
        ad.set_subgrids([])
        ad.update_samples(level0[k])
        ad.set_subgrids(subs[k])
        capi.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    out["three_call_wall_ms"], out["three_call_wall_min_ms"] = med(wall[warmup:]), round(min(wall[warmup:]), 3)
    out["n_blocks"], out["n_blocks_empty"] = ad.info()["n_blocks"], ad.info()["n_blocks_empty"]
    if three_call_only:
        return out
    bare = HipVolumeAdapter(vol, 2.0)  # no transfer function: its update is ranges + download alone
    wall, ms, ms_bare, ms_kernel = [], [], [], []
    for i in range(warmup + steps):  # profiling off: the wall time and both ms_out
        k = (i + 1) % 2
        t0 = time.perf_counter()
        ms.append(ad.update_amr(level0[k], subs[k]))
        wall.append((time.perf_counter() - t0) * 1e3)
        ms_bare.append(bare.update_amr(level0[k], subs[k]))
    out["n_blocks_empty_in_place"] = ad.info()["n_blocks_empty"]  # (the same step as the three-call loop ended on: the same count)
    capi.profile(1)
    for i in range(warmup + steps):  # a pass of its own for the range kernels' event time
        k0 = capi.stats()["ms_build"]
        ad.update_amr(level0[(i + 1) % 2], subs[(i + 1) % 2])
        ms_kernel.append(capi.stats()["ms_build"] - k0)
    capi.profile(0)
    w = warmup
    out.update({"update_wall_ms": med(wall[w:]), "update_wall_min_ms": round(min(wall[w:]), 3), "update_wall_max_ms": round(max(wall[w:]), 3),
                "update_ms_out": med(ms[w:]), "uploads_ms": med(np.array(wall[w:]) - np.array(ms[w:])), "range_kernels_ms": med(ms_kernel[w:]),
                "ranges_and_download_ms": med(ms_bare[w:]), "table_rebuild_ms": med(np.array(ms[w:]) - np.array(ms_bare[w:])),
                "three_call_over_update": round(out["three_call_wall_ms"] / max(float(np.median(wall[w:])), 1e-9), 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rate", type=float, default=1.0)
    ap.add_argument("--tf", nargs="+", default=["thin", "spikes"])
    ap.add_argument("--json")
    ap.add_argument("--surfaces", action="store_true")
    ap.add_argument("--update", action="store_true")
    ap.add_argument("--clip", action="store_true")
    ap.add_argument("--shade", action="store_true")
    ap.add_argument("--gradient", choices=["cell", "central"], default="cell",
                    help="with --shade: central = the lit and the isosurface frame with both gradient kinds; with --fused: central = those two frames with CENTRAL "
                         "bricks, fused against the loop, and with --shadows / --fog-shadows / --mesh-shadows the shadowed frames, CENTRAL against CELL")
    ap.add_argument("--amr", action="store_true")
    ap.add_argument("--recreate-only", action="store_true")
    ap.add_argument("--three-call-only", action="store_true", help="with --update --amr: the three-call route alone")
    ap.add_argument("--domains", type=int, nargs="+", metavar="W")
    ap.add_argument("--per-queue", action="store_true")
    ap.add_argument("--overlap", action="store_true")
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="f32")
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--bricks", type=int, nargs="+", choices=sorted(FUSED_SPLITS), default=sorted(FUSED_SPLITS), help="with --fused: the brickings")
    ap.add_argument("--shadows", action="store_true", help="with --fused --surfaces: the shadowed frame against the shaded fused frame")
    ap.add_argument("--bias", type=int, default=2, help="with --shadows: the first shadow sample's lattice index")
    ap.add_argument("--fog-shadows", action="store_true", help="with --fused --shade: the lit fused frame against the fog-shadowed frame, and the bake of its light grids")
    ap.add_argument("--mesh-shadows", action="store_true", help="with --fused --shade --fog-shadows: the fog-shadowed frame against the mesh-shadowed frame, and the bake of its occluder grids")
    ap.add_argument("--ao", action="store_true", help="with --fused --shade --fog-shadows [--mesh-shadows] [--surfaces] [--gradient central]: the base frame against the AO frame, "
                                                      "and the bake of the AO grid beside the light grids'")
    ap.add_argument("--ao-dirs", type=int, default=16, help="with --ao: directions of the bake (Fibonacci sphere)")
    a = ap.parse_args()
    if a.update or a.domains:
        import torch  # noqa: F401  (the device samples; imported before the library initialises the device)
    capi.init(0)
    out = {"source_hash": _build.source_hash(), "width": 1920, "height": 1080, "runs": []}
    if a.update and a.amr:
        for n in ([256] if a.sizes == [256, 512] else a.sizes):
            for device in (False, True):
                r = run_amr_update(n, device, a.steps, a.warmup, a.three_call_only)
                out["runs"].append(r)
                print(json.dumps(r), flush=True)
        a.sizes = []
        a.update = a.amr = False
    if a.update:
        for n in a.sizes:
            for device in (False, True):
                r = run_update(n, device, a.steps, a.warmup, a.recreate_only, a.dtype)
                out["runs"].append(r)
                print(json.dumps(r), flush=True)
        a.sizes = []
    if a.domains:
        for n in ([256] if a.sizes == [256, 512] else a.sizes):
            vol = noise(n, "f32")
            for split in ((2, 2, 2), (4, 4, 4)):
                r = run(n, split, a.steps, a.warmup, a.rate, "thin", vol)  # the one-rank native frame of the same bricks
                r["mode"] = "one_rank_native"
                out["runs"].append(r)
                print(json.dumps(r), flush=True)
                for w in a.domains:
                    for per_queue in ((False, True) if a.per_queue else (False,)):
                        r = run_domains(n, split, w, a.steps, a.warmup, a.rate, "thin", vol, per_queue, a.overlap)
                        out["runs"].append(r)
                        print(json.dumps(r), flush=True)
        a.sizes = []
    if a.fused and a.amr and (a.shadows or a.fog_shadows or a.mesh_shadows):  # shadows on AMR bricks against the same frames without subgrids
        if not (a.surfaces and a.shade):
            ap.error("--amr with --shadows / --fog-shadows / --mesh-shadows goes with --fused --surfaces --shade")
        frames = ([("shadowed", "surf")] if a.shadows else []) + ([("fog", "lit"), ("fog", "surf_lit")] if a.fog_shadows else [])
        frames += [("mesh", "lit"), ("mesh", "surf_lit")] if a.mesh_shadows else []
        for n in ([256] if a.sizes == [256, 512] else a.sizes):
            vol = amr_bricked_scene(n)
            for frame, shape in frames:
                first = None
                for nb in a.bricks:
                    r, fb = run_shadow_amr(n, FUSED_SPLITS[nb], a.steps, a.warmup, 2.0 if a.rate == 1.0 else a.rate, vol, frame, shape, first)
                    first = fb if first is None else first
                    out["runs"].append(r)
                    print(json.dumps(r), flush=True)
        a.sizes = []
        a.shadows = a.fog_shadows = a.mesh_shadows = False
    elif a.fused and a.amr:  # the fused AMR frame against the loop and against the subgrid-free fused frame
        for n in ([256] if a.sizes == [256, 512] else a.sizes):
            vol = amr_bricked_scene(n)
            for shaded in ([None] if not (a.surfaces or a.shade) else (["surfaces"] if a.surfaces else []) + (["lit"] if a.shade else [])):
                for nb in a.bricks:
                    r = run_fused_amr(n, FUSED_SPLITS[nb], a.steps, a.warmup, 2.0 if a.rate == 1.0 else a.rate, vol, shaded)
                    out["runs"].append(r)
                    print(json.dumps(r), flush=True)
        a.sizes = []
    elif a.amr and (a.surfaces or a.shade):  # the shaded AMR frame against the plain volume's shaded frame and against the plain AMR frame
        for n in ([256] if a.sizes == [256, 512] else a.sizes):
            for what in (["surfaces"] if a.surfaces else []) + (["shade"] if a.shade else []):
                r = run_amr_shaded(n, a.steps, a.warmup, 2.0 if a.rate == 1.0 else a.rate, what)
                out["runs"].append(r)
                print(json.dumps(r), flush=True)
        a.sizes = []
    elif a.amr:
        for n in ([256] if a.sizes == [256, 512] else a.sizes):
            for r in run_amr(n, a.steps, a.warmup, 2.0 if a.rate == 1.0 else a.rate):
                out["runs"].append(r)
                print(json.dumps(r), flush=True)
        a.sizes = []
    if a.shadows and not (a.fused and a.surfaces):
        ap.error("--shadows goes with --fused --surfaces")
    if a.fog_shadows and not (a.fused and a.shade):
        ap.error("--fog-shadows goes with --fused --shade")
    if a.mesh_shadows and not a.fog_shadows:
        ap.error("--mesh-shadows goes with --fused --shade --fog-shadows")
    if a.ao:  # ambient occlusion: its own rows, and nothing else
        if not (a.fused and a.shade and a.fog_shadows):
            ap.error("--ao goes with --fused --shade --fog-shadows")
        for n in a.sizes:
            vol = noise(n, a.dtype)
            for shape, kind in [("lit", k) for k in a.tf] + ([("surf_lit", "thin")] if a.surfaces else []):
                first = None
                for nb in a.bricks:
                    r, fb = run_ao(n, FUSED_SPLITS[nb], a.steps, a.warmup, a.rate, kind, vol, shape, a.dtype, first, a.mesh_shadows, a.gradient == "central", a.ao_dirs)
                    first = fb if first is None else first
                    out["runs"].append(r)
                    print(json.dumps(r), flush=True)
        a.sizes = []
    if a.fused and a.gradient == "central":  # the CENTRAL rows, ahead of the rows the other flags print: fused against the loop, and the shadowed frames asked for against their CELL frames
        for n in a.sizes:
            vol = noise(n, a.dtype)
            for what, kind in [("lit", k) for k in a.tf] + [("iso", "thin")]:
                for nb in a.bricks:
                    r = run_fused_central(n, FUSED_SPLITS[nb], a.steps, a.warmup, a.rate, kind, vol, what, a.dtype)
                    out["runs"].append(r)
                    print(json.dumps(r), flush=True)
            for which, on in zip(CENTRAL_FRAMES, (a.shadows, a.fog_shadows, a.mesh_shadows)):
                first = None
                for nb in a.bricks if on else ():
                    r, fb = run_central_shadows(n, FUSED_SPLITS[nb], a.steps, a.warmup, a.rate, "thin", vol, which, a.dtype, first)
                    first = fb if first is None else first
                    out["runs"].append(r)
                    print(json.dumps(r), flush=True)
    for n in a.sizes if a.shadows else ():
        vol = noise(n, a.dtype)
        first = None
        for nb in a.bricks:
            r, fb = run_shadows(n, FUSED_SPLITS[nb], a.steps, a.warmup, a.rate, vol, a.dtype, first, a.bias)
            first = fb if first is None else first
            out["runs"].append(r)
            print(json.dumps(r), flush=True)
    if a.shadows:
        a.sizes = []
    for n in a.sizes if a.mesh_shadows else ():
        vol = noise(n, a.dtype)
        for shape, kind in [("lit", k) for k in a.tf] + ([("surf_lit", "thin"), ("surf", "thin")] if a.surfaces else []):
            first = None
            for nb in a.bricks:
                r, fb = run_mesh_shadows(n, FUSED_SPLITS[nb], a.steps, a.warmup, a.rate, kind, vol, shape, a.dtype, first)
                first = fb if first is None else first
                out["runs"].append(r)
                print(json.dumps(r), flush=True)
    if a.mesh_shadows:
        a.sizes = []
    for n in a.sizes if a.fog_shadows else ():
        vol = noise(n, a.dtype)
        for kind in a.tf:
            first = None
            for nb in a.bricks:
                r, fb = run_fog_shadows(n, FUSED_SPLITS[nb], a.steps, a.warmup, a.rate, kind, vol, a.dtype, first)
                first = fb if first is None else first
                out["runs"].append(r)
                print(json.dumps(r), flush=True)
    if a.fog_shadows:
        a.sizes = []
    for n in a.sizes if a.fused else ():
        vol = noise(n, a.dtype)
        cases = [(None, kind) for kind in a.tf]
        if a.surfaces or a.shade:  # the shaded fused frame
            cases = ([("surfaces", "thin")] if a.surfaces else []) + ([("lit", kind) for kind in a.tf] if a.shade else [])
        for shaded, kind in cases:
            for nb in a.bricks:
                r = run_fused(n, FUSED_SPLITS[nb], a.steps, a.warmup, a.rate, kind, vol, a.dtype, shaded)
                out["runs"].append(r)
                print(json.dumps(r), flush=True)
    if a.fused:
        a.sizes = []
    for n in a.sizes if a.clip else ():
        vol = noise(n, a.dtype)
        for fn in (run_clip, run_mixed):
            for split in ((1, 1, 1), (2, 2, 2)):
                r = fn(n, split, a.steps, a.warmup, a.rate, vol, a.dtype)
                out["runs"].append(r)
                print(json.dumps(r), flush=True)
    if a.clip:
        a.sizes = []
    for n in a.sizes if a.shade else ():
        vol = noise(n, a.dtype)
        for kind in a.tf:
            for split in ((1, 1, 1), (2, 2, 2)):
                r = (run_smooth if a.gradient == "central" else run_shade)(n, split, a.steps, a.warmup, a.rate, kind, vol, a.dtype)
                out["runs"].append(r)
                print(json.dumps(r), flush=True)
    if a.shade:
        a.sizes = []
    for n in a.sizes if a.surfaces else ():
        vol = noise(n, a.dtype)
        for split in ((1, 1, 1), (2, 2, 2)):
            base = None
            for mode, iso in SURFACE_MODES.items():
                r = run(n, split, a.steps, a.warmup, a.rate, "thin", vol, iso, a.dtype)
                r["mode"] = mode
                base = r["ms_median"] if mode == "plain" else base
                r["vs_plain"] = round(r["ms_median"] / base, 3)
                out["runs"].append(r)
                print(json.dumps(r), flush=True)
    for n in () if a.surfaces else a.sizes:
        vol = noise(n, a.dtype)  # (once per size: the 512^3 grid takes longer to make than to render)
        for kind in a.tf:
            for split in ((1, 1, 1), (2, 2, 2)):
                r = run(n, split, a.steps, a.warmup, a.rate, kind, vol, dtype=a.dtype)
                out["runs"].append(r)
                print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
