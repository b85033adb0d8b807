"""Meshes under instance matrices with rotation, shear and mirroring (tests/affine_cases.py) on the device: Adapter::trace against the oracle
bit for bit and against a float64 world-space brute force, the same call under the knobs that reach the other traversal kernels (with the
counters that show they ran), one-instance and many-instance frames through the native Image and Domain schedulers against the oracle's
restated loops, and a rigid motion frame by frame through update_scene / set_transforms.  The oracle's matrix arithmetic is pinned to the
reference's glm by tests/test_affine_host.py; what differs from the oracle here is the device's."""
import numpy as np
import pytest

from gravit_amd import scenes
from gravit_amd.adapter import HipMeshAdapter
from gravit_amd.layouts import BLINN, LAMBERT, NORMALS_FLAT, NORMALS_SMOOTH, PHONG, RAY_DTYPE, RAY_EPSILON, ambient_light, area_light, default_material, point_light
from gravit_amd.scheduler import NativeTracer
from oracle import orc
from tests import affine_cases as ac
from tests.helpers import oracle_render, oracle_render_domain, rays_equal_bits, sort_rays
from tests.test_gpu_native import run_native_ranks

pytestmark = pytest.mark.gpu

F = np.float32
FLT_MAX = np.finfo(F).max


def fuzz_case(family, variant, n_rays=None):
    """test_random_adapter_calls_against_the_oracle's recipe under a matrix of `family`: a random mesh, one to three lights (point, ambient,
    area), rays of all three types aimed near triangle centroids from 4 units away, with random depth, weight, colour and t."""
    rng = np.random.default_rng([41000, ac.FAMILIES.index(family), variant])
    n_v, n_t = int(rng.integers(60, 900)), int(rng.integers(200, 1800))
    v = rng.normal(size=(n_v, 3)).astype(F)
    t = rng.integers(0, n_v, (n_t, 3)).astype(np.int32)
    mtype = (LAMBERT, LAMBERT, PHONG, BLINN)[variant % 4]
    mat = default_material(kd=rng.uniform(0.1, 0.9, 3), mtype=mtype, ks=rng.uniform(0.1, 0.9, 3), alpha=float(rng.uniform(1.0, 30.0)))
    mode = NORMALS_SMOOTH if variant % 2 else NORMALS_FLAT
    vnrm = None
    if variant % 4 == 3:  # the caller's own vertex normals (not generated)
        vnrm = rng.normal(size=(n_v, 3)).astype(F)
        vnrm /= np.linalg.norm(vnrm, axis=1, keepdims=True)
    m = ac.matrix(family, 10 + variant)
    lights = [point_light(rng.uniform(-6, 6, 3), rng.uniform(0.2, 1.0, 3))]
    if variant % 3 == 1:
        lights.append(ambient_light(rng.uniform(0.05, 0.3, 3)))
    if variant % 3 == 2:
        lights.append(area_light(rng.uniform(-6, 6, 3), rng.uniform(0.2, 1.0, 3), (0.0, -1.0, 0.0), 0.7, 0.4))
        lights.append(point_light(rng.uniform(-6, 6, 3)))
    n = n_rays or int(rng.integers(2500, 5000))
    rays = np.zeros(n, RAY_DTYPE)
    rays["origin"], rays["direction"] = ac.centroid_rays(m, v, t, n, 100 * ac.FAMILIES.index(family) + variant)
    rays["t_min"], rays["t_max"], rays["t"] = RAY_EPSILON, FLT_MAX, rng.uniform(0.1, 5.0, n).astype(F)
    rays["type"] = rng.choice([0, 0, 1, 2], n)
    rays["depth"], rays["w"], rays["id"] = rng.choice([1, 1, 2, 3], n), rng.uniform(0.05, 1.0, n).astype(F), rng.integers(0, 1 << 20, n)
    rays["color"] = rng.uniform(0, 1, (n, 3)).astype(F)
    rays["rng"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    begin = int(rng.integers(0, n // 3))
    end = 0 if variant % 4 == 0 else int(rng.integers(begin + n // 2, n + 1))
    return dict(v=v, t=t, mat=mat, mtype=mtype, mode=mode, vnrm=vnrm, m=m, lights=np.concatenate(lights), rays=rays, begin=begin, end=end)


def assert_trace_equals_oracle(c, rg, out_g, rc, out_c):
    assert len(out_g) == len(out_c)
    a, b = sort_rays(out_g), sort_rays(out_c)
    if c["mtype"] == LAMBERT:
        assert rays_equal_bits(a, b) and rays_equal_bits(rg, rc)
    else:  # powf
        for f in RAY_DTYPE.names:
            if f == "color":
                assert np.abs(a[f] - b[f]).max(initial=0.0) <= 1e-5
            else:
                assert a[f].tobytes() == b[f].tobytes(), f
        assert rays_equal_bits(rg, rc)


@pytest.mark.parametrize("variant", range(4))
@pytest.mark.parametrize("family", ac.FAMILIES)
def test_adapter_calls_under_every_matrix_family(hip, family, variant):
    """Adapter::trace under a full matrix: moved rays as a set and the list in place equal orc.Mesh.trace bit for bit (the powf materials
    within 1e-5); and on the same rays the device's t equals the float64 world-space brute force of tests/affine_cases.py: hit / miss for
    every ray, median relative error below 1e-6, at most 1 % of the rays above 1e-4."""
    c = fuzz_case(family, variant)
    mesh = scenes.MeshData(c["v"], c["t"], c["mat"], vnormals=c["vnrm"])
    ad, om = HipMeshAdapter(mesh, c["mode"]), orc.Mesh(c["v"], c["t"], vnormals=c["vnrm"], mesh_mat=c["mat"])
    minv, normi = scenes.instance_matrices(c["m"])
    rays, begin, end = c["rays"], c["begin"], c["end"]
    rg, rc = rays.copy(), rays.copy()
    out_g = ad.trace(rg, c["m"], minv, normi, c["lights"], begin=begin, end=end, seed=variant)
    out_c = om.trace(rc, c["m"], minv, normi, c["lights"], c["mode"], seed=variant, begin=begin, end=end)
    assert_trace_equals_oracle(c, rg, out_g, rc, out_c)
    assert len(out_g) > 20
    sel = np.zeros(len(rays), bool)
    sel[begin:(end or len(rays))] = True
    sel &= (rays["type"] != 1) & (rays["depth"] == 1)  # a shadow ray that hits is dropped, its t not written; a ray with depth left may bounce and be traced again
    t64 = ac.world_hits64(c["m"], c["v"], c["t"], rays["origin"][sel], rays["direction"][sel], float(RAY_EPSILON))
    got = np.where(rg["t"][sel].view(np.uint32) != rays["t"][sel].view(np.uint32), rg["t"][sel], FLT_MAX)
    wrong, median, share = ac.check_against_world(got, t64)
    print("%s %d: %d rays, %d hits, %d disagreements, median rel %.3g, share above 1e-4 %.4f" % (family, variant, sel.sum(), np.isfinite(t64).sum(), wrong, median, share))
    assert np.isfinite(t64).sum() > 300
    assert wrong == 0 and median < 1e-6 and share <= 0.01
    outside = ~np.zeros(len(rays), bool)
    outside[begin:(end or len(rays))] = False
    assert rays_equal_bits(rg[outside], rays[outside])


KNOBS = [dict(sort_rays=1), dict(long_steps=2, long_min_rays=0), dict(long_steps=0), dict(term_sink=0), dict(leaf_max=1), dict(leaf_max=3),
         dict(leaf_max=4, long_steps=4, long_min_rays=0)]


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_adapter_call_under_the_knobs_that_reach_the_other_kernels(hip, family):
    """The adapter call of one family under test_results_do_not_depend_on_tuning_knobs' knobs -- sorted lists (the sort takes the
    ray through minv for its keys), parked rays finished a wave per ray (k_long_closest), no parking, no sink, leaves of 1 / 3 / 4 --
    with the evidence that the path ran: the sort's time, the parked-ray counter word and k_long_closest's time, the mesh's leaf size.  8,209 rays: a list below
    8,192 is never sorted (trace_core)."""
    c = fuzz_case(family, 1, n_rays=8209)
    mesh = scenes.MeshData(c["v"], c["t"], c["mat"])
    om = orc.Mesh(c["v"], c["t"], mesh_mat=c["mat"])
    minv, normi = scenes.instance_matrices(c["m"])
    rc = c["rays"].copy()
    out_c = om.trace(rc, c["m"], minv, normi, c["lights"], c["mode"], seed=3)
    for opts in KNOBS:
        try:
            for k, v in opts.items():
                hip.set_option(k, v)
            ad = HipMeshAdapter(mesh, c["mode"])  # after the options: leaf_max is a build-time knob of the mesh
            assert ad.info()["max_leaf"] == opts.get("leaf_max", 2)
            hip.stats_reset(); hip.profile(1)
            rg = c["rays"].copy()
            out_g = ad.trace(rg, c["m"], minv, normi, c["lights"], seed=3)
            st, parked = hip.stats(), int(hip.counters_peek()[3])
            hip.profile(False)
            assert_trace_equals_oracle(c, rg, out_g, rc, out_c)
            assert (st["ms_sort"] > 0.0) == bool(opts.get("sort_rays", 0)), opts
            if opts.get("long_min_rays", 1) == 0:
                assert parked > 0 and st["ms_long"] > 0.0, (opts, parked)  # rays were parked and finished a wave per ray
            if opts.get("long_steps", 1) == 0:
                assert parked == 0 and st["ms_long"] == 0.0, opts
        finally:
            hip.profile(False)
            hip.set_option("defaults", 0)


def one_instance_scene(family, seed=0):
    v, t = ac.random_mesh(20 + seed, 300, 1200)
    mesh = scenes.MeshData((v * F(0.3)).astype(F), t, default_material(kd=(0.7, 0.6, 0.5)))
    m = ac.matrix(family, 30 + seed)
    M = m.reshape(4, 4).T.astype(np.float64)
    w = mesh.verts.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    c = w.mean(axis=0)
    lo, hi = scenes.instance_bbox(m, *mesh.bbox())
    far = 1.1 * float(np.linalg.norm(hi.astype(np.float64) - lo))  # outside the instance's box (no ray is assigned to a box it starts in)
    eye = tuple(c + far * np.array([0.1, 0.2, 0.97]))
    fov = 2.0 * np.arctan(2.2 * float(np.median(np.linalg.norm(w - c, axis=1))) / far)  # the blob fills the film; the light stands at the eye
    cam = scenes.Camera(eye, tuple(c), (0.0, 1.0, 0.0), float(fov), 64, 48)
    return scenes._assemble([mesh], [0], [m], point_light(eye), cam, "affine-one-" + family)


CW_LONG, CW_PACKETS = 3, 9  # counter words (csrc/gvt_device.h): rays handed to k_long_closest by the last closest-hit launch; packets that k_packet gave up on this frame
PINNED = dict(finish_auto=0, finish_rays=0, long_auto=0)  # no k_finish, no route probing, no moving threshold: the knobs below decide the kernels


def routed_frame(hip, sc, mode, opts, frames=1):
    """A NativeTracer frame of sc under opts with profiling on: (framebuffer, frame stats, library stats, counter words)."""
    try:
        for k, v in opts.items():
            hip.set_option(k, v)
        hip.stats_reset(); hip.profile(1)
        tr = NativeTracer(sc, mode)
        for _ in range(frames):
            fb = tr().framebuffer(True).copy()
        out = fb, dict(tr.stats), hip.stats(), hip.counters_peek()
        tr.close()
        return out
    finally:
        hip.profile(False)
        hip.set_option("defaults", 0)


# the single-mesh chain's routes (trace.hip single_pass).  A 64 x 48 film is 3,072 rays: at the default small_rays = 4096 every round goes a wave per ray,
# so the lane and packet kernels need small_rays = 0
ONE_ROUTES = {
    "waves": dict(PINNED),                                                       # k_long_closest / k_wave_any over every ray
    "lanes": dict(PINNED, small_rays=0, packet=0, long_min_rays=0),              # k_trace XFORM (+ parked rays), the early-deposit any-hit launch (MODE 2)
    "lanes_late": dict(PINNED, small_rays=0, packet=0, long_min_rays=0, early_deposit=0),  # ... and k_trace's plain any-hit launch (MODE 1)
    "lanes_no_sink": dict(PINNED, small_rays=0, packet=0, long_min_rays=0, term_sink=0),
    "packets": dict(PINNED, small_rays=0, packet=2, packet_min_rays=0),          # k_packet for the closest and the any hit
}


@pytest.mark.parametrize("route", sorted(ONE_ROUTES))
@pytest.mark.parametrize("mode", [NORMALS_FLAT, NORMALS_SMOOTH])
@pytest.mark.parametrize("family", ac.FAMILIES)
def test_one_instance_frames(hip, family, mode, route):
    """One instance under a full matrix through the native tracer, on each route of the single-mesh chain -- a wave per ray (the default at
    this film size), k_trace's XFORM path with the `translation x 0` terms in scalar registers and its early-deposit any-hit launch, the
    same with the plain any-hit launch, k_packet -- with the lean k_shade: the oracle's image and ray counts, bit for bit.  Which of the
    closest-hit step's three modes ran (trace.hip closest_step) is read from the counters: only the lane mode launches k_long_closest under
    its own heading (ms_long, with long_min_rays = 0), the wave mode seeds every ray of the list into word 3, and the packet mode does
    neither (word 3 then holds the rays of packets that gave up, word 9 those packets: no counter counts the packets walked); the
    early-deposit launches are counted by the frame.  That the packet mode's transform is k_packet's own was checked with a transposition
    of packet_kernel.inc's product on a scratch copy: only this route's cases fail."""
    sc = one_instance_scene(family)
    ref, st = oracle_render(sc, mode, nthreads=8)
    assert (ref[..., :3].sum(axis=2) > 0).sum() > 300 and st.rays_any > 300
    fb, fs, ls, words = routed_frame(hip, sc, mode, ONE_ROUTES[route])
    assert np.array_equal(fb[..., :3].view(np.uint32), ref[..., :3].view(np.uint32)) and np.array_equal(fb[..., 3], ref[..., 3])
    assert fs["rays_closest"] == st.rays_closest and fs["rays_any"] == st.rays_any
    print(route, "packets", words[CW_PACKETS], "long", words[CW_LONG], "ms_long", ls["ms_long"], "early", fs["early_deposit_launches"], "chains", fs["chains"])
    if route == "packets":
        assert ls["ms_long"] == 0.0 and words[CW_LONG] <= 64 * words[CW_PACKETS] < 300 and fs["early_deposit_launches"] == 0
    elif route == "waves":
        assert words[CW_PACKETS] == 0 and ls["ms_long"] == 0.0 and words[CW_LONG] > 300 and fs["early_deposit_launches"] == 0
    else:
        assert words[CW_PACKETS] == 0 and ls["ms_long"] > 0.0
        assert (fs["early_deposit_launches"] > 0) == (route == "lanes")


def instances_seen(sc):
    """Per instance: the camera rays whose float64 world-space hit with that instance alone exists."""
    rays = orc.camera_rays(sc.camera.eye, sc.camera.focus, sc.camera.up, sc.camera.fov, sc.camera.width, sc.camera.height)
    return [int(np.isfinite(ac.world_hits64(sc.m[i], sc.meshes[sc.inst_mesh[i]].verts, sc.meshes[sc.inst_mesh[i]].tris, rays["origin"], rays["direction"])).sum())
            for i in range(sc.n_inst)]


@pytest.fixture(scope="module")
def mixed():
    sc = ac.mixed_scene(0, 8)
    refs = {mode: oracle_render(sc, mode, nthreads=8) for mode in (NORMALS_FLAT, NORMALS_SMOOTH)}
    return sc, refs


def test_the_mixed_scene_shows_every_instance(mixed):
    sc, refs = mixed
    ref, st = refs[NORMALS_FLAT]
    assert (ref[..., :3].sum(axis=2) > 0).sum() > 300
    assert min(instances_seen(sc)) > 0  # every instance is hit by camera rays (its queue receives rays)
    assert sorted({ac.FAMILIES[i % 6] for i in range(sc.n_inst)}) == sorted(ac.FAMILIES)


@pytest.mark.parametrize("opts", [dict(), dict(small_rays=0), dict(small_rays=1 << 30), dict(finish_rays=0), dict(finish_rays=1 << 30), dict(term_sink=0), dict(hop_local=0), dict(hop_local=2),
                                  dict(leaf_max=4, small_rays=0), dict(sort_rays=1), dict(packet=1, packet_min_rays=0)])
@pytest.mark.parametrize("mode", [NORMALS_FLAT, NORMALS_SMOOTH])
def test_mixed_frames_on_one_rank(hip, mixed, mode, opts):
    """Eight instances of two meshes, all six families, overlapping boxes (from the eight-corner scenes.instance_bbox), through the
    native Image scheduler on one rank: k_top_classify / k_top_scatter, the merged k_shade, both multi-instance lookups of k_trace, the
    hop into the next local instance and k_finish or per-hop rounds (finish_rays), a wave per ray or never (small_rays): the oracle's image
    bit for bit, its ray counts, frame after frame (finish_auto's probing frames included)."""
    sc, refs = mixed
    ref, st = refs[mode]
    try:
        for k, v in opts.items():
            hip.set_option(k, v)
        tr = NativeTracer(sc, mode)
        chains = []
        for _ in range(4 if not opts else 2):
            fb = tr().framebuffer(True)
            assert np.array_equal(fb[..., :3].view(np.uint32), ref[..., :3].view(np.uint32)) and np.array_equal(fb[..., 3], ref[..., 3]), opts
            assert tr.stats["rays_closest"] == st.rays_closest and tr.stats["rays_any"] == st.rays_any, opts
            chains.append(tr.stats["chains"])
        tr.close()
    finally:
        hip.set_option("defaults", 0)
    print(opts, "chains", chains)


def test_finish_kernel_and_per_hop_rounds_both_run_on_the_mixed_scene(hip, mixed):
    """The evidence for the two routes above, as test_small_rounds_through_one_launch_or_per_hop_... reads it: with k_finish pinned off a
    frame whose rays hop between instances needs more launch chains than with it pinned on."""
    sc, refs = mixed
    chains = {}
    for fin in (1 << 30, 0):
        try:
            hip.set_option("finish_auto", 0); hip.set_option("finish_rays", fin); hip.set_option("hop_local", 0)
            tr = NativeTracer(sc, NORMALS_FLAT)
            fb = tr().framebuffer(True)
            assert np.array_equal(fb[..., :3].view(np.uint32), refs[NORMALS_FLAT][0][..., :3].view(np.uint32))
            chains[fin] = tr.stats["chains"]
            tr.close()
        finally:
            hip.set_option("defaults", 0)
    assert chains[0] > chains[1 << 30], chains


# the merged chain's routes (trace.hip merged_pass).  At this film size a round is below the default small_rays and finish_rays, so without these
# knobs every round ends in k_finish or goes a wave per ray
MANY_ROUTES = {
    "lanes": dict(PINNED, small_rays=0, long_min_rays=0, hop_local=0),            # k_trace<MULTI> for the closest and the any hit
    "lanes_packet_off": dict(PINNED, small_rays=0, long_min_rays=0, hop_local=0, packet=0),
    "lanes_hops": dict(PINNED, small_rays=0, long_min_rays=0, hop_local=2),       # ... a ray that misses goes on into the next instance inside the launch
    "lanes_hops_early": dict(PINNED, small_rays=0, long_min_rays=0, hop_local=3),
    "packets": dict(PINNED, small_rays=0, hop_local=0, packet=2, packet_min_rays=0),  # k_packet_multi for the camera's round (long_min_rays left alone: no k_long_closest heading)
    "waves": dict(PINNED, hop_local=0),
    "waves_hops": dict(PINNED, hop_local=2),
}


@pytest.fixture(scope="module")
def crowd():
    """40 instances: more than the 32 the lane kernel keeps in its LDS table, so it looks every instance up in the round's table in memory."""
    sc = ac.mixed_scene(1, 40)
    return sc, {mode: oracle_render(sc, mode, nthreads=8) for mode in (NORMALS_FLAT, NORMALS_SMOOTH)}


@pytest.mark.parametrize("route", sorted(MANY_ROUTES))
@pytest.mark.parametrize("mode", [NORMALS_FLAT, NORMALS_SMOOTH])
@pytest.mark.parametrize("which", ["mixed", "crowd"])
def test_many_instance_frames_on_every_route_of_the_merged_chain(hip, mixed, crowd, which, mode, route):
    """The merged chain with k_finish pinned off, on each of its routes: the lane-per-ray k_trace<MULTI> -- whose instance lookup goes through
    the LDS table with 8 instances (mixed) and through the round's table in memory with 40 (crowd: more than KT_TAB = 32) --, with and without
    hops inside the launch, k_packet_multi, and a wave per ray: the oracle's image and ray counts, bit for bit, two frames.  The route is read
    from the counters as in test_one_instance_frames (lanes: k_long_closest's own heading ran; waves and packets: it did not).  Which
    lookup the lane kernel took follows from the instance count alone, and that k_packet_multi, the LDS table and the table in memory each
    carry the rays was checked with a transposition at each site on a scratch copy: packet_kernel.inc's multi product fails only the
    packet route, trace_lane.inc's s_inst product only the lane routes of `mixed`, its W.insts product only those of `crowd`."""
    sc, refs = mixed if which == "mixed" else crowd
    assert (sc.n_inst > 32) == (which == "crowd")
    ref, st = refs[mode]
    assert (ref[..., :3].sum(axis=2) > 0).sum() > 300
    fb, fs, ls, words = routed_frame(hip, sc, mode, MANY_ROUTES[route], frames=2)
    assert np.array_equal(fb[..., :3].view(np.uint32), ref[..., :3].view(np.uint32)) and np.array_equal(fb[..., 3], ref[..., 3])
    assert fs["rays_closest"] == st.rays_closest and fs["rays_any"] == st.rays_any
    print(which, route, "packets", words[CW_PACKETS], "long", words[CW_LONG], "ms_long", ls["ms_long"], "chains", fs["chains"])
    if route == "packets" or route.startswith("waves"):
        assert ls["ms_long"] == 0.0
    else:
        assert words[CW_PACKETS] == 0 and ls["ms_long"] > 0.0
    if route == "lanes_hops":
        assert fs["chains"] < routed_frame(hip, sc, mode, MANY_ROUTES["lanes"])[1]["chains"]  # hops inside the launch save rounds


@pytest.mark.parametrize("bsp", [True, False])
@pytest.mark.parametrize("world", [2, 3])
def test_mixed_frames_under_the_domain_scheduler(hip, mixed, world, bsp):
    """The same scene with its instances dealt round-robin to two and three in-process ranks, BSP rounds and overlapped ticks, against
    the oracle's restated DomainTracer: the composited image bit for bit, rays sent and traced equal, and rays do change rank."""
    sc, refs = mixed
    owner = [i % world for i in range(sc.n_inst)]
    refd, std = oracle_render_domain(sc, owner, world, NORMALS_SMOOTH)
    assert np.array_equal(refd[..., :3].view(np.uint32), refs[NORMALS_SMOOTH][0][..., :3].view(np.uint32))  # the schedulers agree on the image
    res = run_native_ranks(sc, owner, world, NORMALS_SMOOTH, bsp)
    assert np.array_equal(res[0][0][..., :3].view(np.uint32), refd[..., :3].view(np.uint32)) and np.array_equal(res[0][0][..., 3], refd[..., 3])
    assert std.rays_sent > 0 and sum(r[1]["rays_sent"] for r in res.values()) == std.rays_sent
    assert sum(r[1]["rays_closest"] for r in res.values()) == std.rays_closest and sum(r[1]["rays_any"] for r in res.values()) == std.rays_any


def test_a_rigid_motion_frame_by_frame(hip, mixed):
    """One tracer, six frames: every frame turns each instance a little further about an axis of its own (m_i R_i(frame)) through
    update_scene -- new boxes into the top level, gvt_hip_tracer_set_transforms' rows of minv | normi patched inside the device's instance
    table -- and equals the oracle's frame of a scene built from those matrices, bit for bit.  The fifth frame goes back to the first
    frame's matrices and gives its framebuffer back."""
    sc, _ = mixed
    tr = NativeTracer(sc, NORMALS_SMOOTH)
    shown = {}
    for k, frame in enumerate([0, 1, 2, 3, 0, 4]):
        now = scenes._assemble(sc.meshes, sc.inst_mesh, list(ac.spin(sc, frame)), sc.lights, sc.camera, "spin %d" % frame)
        if k:
            tr.update_scene(now)
        ref, st = oracle_render(now, NORMALS_SMOOTH, nthreads=8)
        fb = tr().framebuffer(True).copy()
        assert np.array_equal(fb[..., :3].view(np.uint32), ref[..., :3].view(np.uint32)) and np.array_equal(fb[..., 3], ref[..., 3]), frame
        assert tr.stats["rays_closest"] == st.rays_closest and tr.stats["rays_any"] == st.rays_any, frame
        if frame in shown:
            assert np.array_equal(fb.view(np.uint32), shown[frame].view(np.uint32))
        shown[frame] = fb
    assert all((shown[f].view(np.uint32) != shown[0].view(np.uint32)).sum() > 100 for f in (1, 2, 3, 4))  # the motion shows
    tr.close()


@pytest.mark.parametrize("mode", [NORMALS_FLAT, NORMALS_SMOOTH])
@pytest.mark.parametrize("family", ac.FAMILIES)
def test_recorded_glm_products_through_the_device(hip, family, mode):
    """The device's xfm_point / xfm_vector against the reference's glm, through a result that exposes them: rays made of the recorded vectors
    (tests/golden/ref_matrix_vectors.json: every vector as origin with every vector as direction, the -0, zero, inf and NaN components
    among them -- the `translation x 0` terms of k_trace's single-instance path) traced by gvt_hip_trace under glm's own m / inverse(m) /
    transpose(inverse(mat3(m))).  The t the call writes into each ray that hits must be, bit for bit, the t of gvt_hip_intersect -- which
    takes no matrix -- on the object-space ray glm recorded for it (inv_point, inv_vector): an ulp in one product moves t.  Hit and miss
    agree for every ray, the inf and NaN rays miss, and the whole call -- the list in place, the moved rays, their shading through the
    recorded normal matrix -- equals the oracle's bit for bit."""
    hits = 0
    for k, row in enumerate(ac.glm_rows(family)):
        o, d, O, D = ac.glm_ray_case(row)
        v, t = ac.targets_mesh(O, D, k)
        mesh = scenes.MeshData(v, t, default_material(kd=(0.6, 0.5, 0.4)))
        ad, om = HipMeshAdapter(mesh, mode), orc.Mesh(v, t, mesh_mat=mesh.material)
        rays = np.zeros(len(o), RAY_DTYPE)
        rays["origin"], rays["direction"] = o, d
        rays["t_min"], rays["t_max"], rays["t"] = RAY_EPSILON, FLT_MAX, FLT_MAX
        rays["depth"], rays["w"], rays["id"] = 1, 1.0, np.arange(len(o))
        light = point_light((5.0, 6.0, 7.0))
        rg, rc = rays.copy(), rays.copy()
        out_g = ad.trace(rg, row["m"], row["inverse"], row["normal_matrix"], light)
        out_c = om.trace(rc, row["m"], row["inverse"], row["normal_matrix"], light, mode)
        h = ad.intersect(O, D, tnear=float(RAY_EPSILON))
        want_t = np.where(h["prim"] >= 0, h["t"], FLT_MAX).astype(F)
        assert np.array_equal(rg["t"].view(np.uint32), want_t.view(np.uint32)), (family, k, np.nonzero(rg["t"].view(np.uint32) != want_t.view(np.uint32))[0])
        special = ~(np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1))
        assert special.sum() >= 36 and (rg["t"][special] == FLT_MAX).all()
        assert len(out_g) == len(out_c) and rays_equal_bits(sort_rays(out_g), sort_rays(out_c)) and rays_equal_bits(rg, rc), (family, k)
        hits += int((h["prim"] >= 0).sum())
    assert hits > 120
