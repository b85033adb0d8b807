"""BASELINE.json's full size (config 3: 10,000,000 random triangles, 1920x1080, primary + shadow) through
size-independent properties, plus a bounded bit-exact sample against the oracle."""
import numpy as np
import pytest

from gravit_amd import scenes
from gravit_amd.adapter import HipMeshAdapter
from gravit_amd.layouts import NORMALS_FLAT
from gravit_amd.scheduler import ImageTracer, NativeTracer
from oracle import orc
from tests.helpers import bits, oracle_camera_rays, oracle_render

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def soup(hip):
    sc = scenes.soup_scene(10_000_000)
    tr = ImageTracer(sc, NORMALS_FLAT)
    return sc, tr


def test_frame_is_reproducible_and_counts_are_consistent(soup, hip):
    sc, tr = soup
    hip.stats_reset()
    fb1 = tr().framebuffer(False).copy()
    st = hip.stats()
    fb2 = tr().framebuffer(False)
    assert np.array_equal(fb1, fb2)  # idempotent: one writer per pixel, no order dependence
    n_primary, n_shadow = st["rays_closest"], st["rays_any"]
    assert n_primary == 1_040_400  # rays whose first domain is the soup's box (1020 x 1020 pixels)
    assert 0.9 * n_primary < n_shadow <= n_primary  # one light: at most one shadow ray per hit
    lit = fb1[..., 3] > 0
    assert lit.sum() <= n_shadow and lit.sum() > 0.5 * n_shadow
    assert fb1[..., :3].max() <= 1.0 and fb1[..., :3].min() >= 0.0
    assert (fb1[..., 3][lit] == 1.0).all()  # exactly one deposit per lit pixel


def test_light_colour_linearity(soup):
    """Radiance is linear in the light colour: halving it halves every pixel exactly (power of two, no clamp)."""
    sc, tr = soup
    a = tr().framebuffer(False)[..., :3].copy()
    old = sc.lights["color"].copy()
    sc.lights["color"] = old * np.float32(0.5)
    try:
        b = tr().framebuffer(False)[..., :3]
    finally:
        sc.lights["color"] = old
    assert np.array_equal(b, a * np.float32(0.5))


def test_hit_records_reconstruct_the_hit_point_and_agree_with_any_hit(soup):
    sc, tr = soup
    ad = next(iter(tr.backend.adapter_cache.values()))
    rays = oracle_camera_rays(sc)[::7]
    h = ad.intersect(rays["origin"], rays["direction"])
    occ = ad.occluded(rays["origin"], rays["direction"])
    assert ((h["prim"] >= 0) == (occ == 1)).all()  # any-hit and closest-hit agree on hit/miss
    hit = h["prim"] >= 0
    assert hit.sum() > 100_000
    m = sc.meshes[0]
    tri = m.verts[m.tris[h["prim"][hit]]].astype(np.float64)
    u, v = h["u"][hit].astype(np.float64)[:, None], h["v"][hit].astype(np.float64)[:, None]
    p_bary = (1 - u - v) * tri[:, 0] + u * tri[:, 1] + v * tri[:, 2]
    p_ray = rays["origin"][hit].astype(np.float64) + rays["direction"][hit].astype(np.float64) * h["t"][hit].astype(np.float64)[:, None]
    assert np.abs(p_bary - p_ray).max() < 2e-5
    assert (h["u"][hit] >= 0).all() and (h["v"][hit] >= 0).all() and (h["u"][hit] + h["v"][hit] <= 1.0 + 1e-6).all()


def test_bounded_sample_bit_exact_against_oracle(soup):
    """~30 K of the frame's rays against the CPU oracle's own BVH over the same 10 M triangles."""
    sc, tr = soup
    ad = next(iter(tr.backend.adapter_cache.values()))
    om = orc.Mesh(sc.meshes[0].verts, sc.meshes[0].tris)
    rays = oracle_camera_rays(sc)[3::67]
    g, c = ad.intersect(rays["origin"], rays["direction"]), om.intersect(rays["origin"], rays["direction"])
    assert (g["prim"] == c["prim"]).all() and (bits(g["t"]) == bits(c["t"])).all()
    assert (bits(g["u"]) == bits(c["u"])).all() and (bits(g["v"]) == bits(c["v"])).all()
    assert (g["prim"] >= 0).sum() > 10_000


def test_traversal_layouts_agree_at_full_size(soup, hip):
    """The default path (compressed 4-wide nodes, long rays parked and finished a wave per ray) and the same without parking return the
    same hit records for every primary ray of the frame, bit for bit -- and the default launch really parked rays."""
    sc, tr = soup
    ad = next(iter(tr.backend.adapter_cache.values()))
    rays = oracle_camera_rays(sc)
    o, d = rays["origin"], rays["direction"]
    hip.stats_reset()
    hip.profile(True)
    try:
        a = ad.intersect(o, d)
        parked_ms = hip.stats()["ms_long"]
        assert 100 < hip.counters_peek()[3] < 100_000  # rays the default launch parked
    finally:
        hip.profile(False)
    hip.set_option("long_steps", 0)
    b = ad.intersect(o, d)
    hip.set_option("defaults", 0)
    assert a.tobytes() == b.tobytes(), "parking long rays changed a hit record"
    assert parked_ms > 0.0 and (a["prim"] >= 0).sum() > 900_000
    assert hip.counters_peek()[3] == 0  # (the last launch, long_steps = 0, parked nothing)


def test_whole_config3_frame_of_the_native_tracer_is_bit_exact(soup, hip):
    """The benchmark's own frame -- 10 M triangles, 1920x1080, the native tracer the bench times -- against a multi-threaded pass of
    the CPU oracle over the same rays: the WHOLE float framebuffer bit for bit, the ray counts equal (the comparison bench.py
    prints as `parity`, inside the test-suite)."""
    sc, _ = soup
    tr = NativeTracer(sc, NORMALS_FLAT)
    fb = tr().framebuffer(True).copy()
    stats = dict(tr.stats)
    fb2 = tr().framebuffer(True)
    assert np.array_equal(fb, fb2)
    ref, st = oracle_render(sc, NORMALS_FLAT, nthreads=16)
    assert fb.shape == ref.shape == (1080, 1920, 4)
    assert np.array_equal(fb.view(np.uint32), ref.view(np.uint32)), "max |diff| %g in %d pixels" % (np.abs(fb - ref).max(), (fb != ref).any(axis=2).sum())
    assert stats["rays_closest"] == st.rays_closest == 1_040_400 and stats["rays_any"] == st.rays_any > 1_000_000
    assert stats["host_syncs"] == 1 and stats["chains"] == 1
    # gvt_hip_profile: 2 brackets the three traversal classes, 3 / 4 one of them (what bench.py's timed steps carry: an event pair costs
    # a few microseconds of the stream); the image does not depend on it
    seen = {}
    for mode in (2, 3, 4):
        hip.stats_reset()
        hip.profile(mode)
        try:
            fb3 = tr().framebuffer(True)
            seen[mode] = hip.stats()
        finally:
            hip.profile(False)
        assert np.array_equal(fb, fb3)
    assert seen[2]["ms_closest"] > 0.3 and seen[2]["ms_any"] > 0.2 and seen[2]["ms_long"] > 0.0
    assert seen[3]["ms_closest"] > 0.3 and seen[3]["ms_any"] == 0.0 and seen[3]["ms_long"] == 0.0
    assert seen[4]["ms_any"] > 0.2 and seen[4]["ms_closest"] == 0.0 and seen[4]["ms_long"] == 0.0
    tr.close()


def test_config1_bunny_conf_at_its_full_film(hip):
    """BASELINE config 1 at the film size data/bunny.conf states (1900 x 1080, :8): three bunny instances through the native tracer
    and through the reference-order loop, whole float framebuffer against the oracle's restated Image scheduler (smooth normals,
    the mode of the reference's golden images)."""
    import os

    from gravit_amd.layouts import NORMALS_SMOOTH
    from tests.conftest import GOLDEN
    sc = scenes.load_conf(os.path.join(GOLDEN, "bunny.conf"))
    assert (sc.camera.width, sc.camera.height) == (1900, 1080)
    ref, st = oracle_render(sc, NORMALS_SMOOTH, nthreads=16)
    assert (ref[..., 3] > 0).sum() > 50_000
    tr = NativeTracer(sc, NORMALS_SMOOTH)
    fb = tr().framebuffer(True)
    assert np.array_equal(fb[..., :3].view(np.uint32), ref[..., :3].view(np.uint32)) and np.array_equal(fb[..., 3], ref[..., 3])
    assert tr.stats["rays_closest"] == st.rays_closest and tr.stats["rays_any"] == st.rays_any
    # three instances: the first chain runs behind the camera filter on device-side counts -- one chain, one host wait for the whole frame
    assert tr.stats["chains"] == 1 and tr.stats["host_syncs"] == 1
    tr.close()
    it = ImageTracer(sc, NORMALS_SMOOTH)
    fb = it().framebuffer(True)
    assert np.array_equal(fb[..., :3].view(np.uint32), ref[..., :3].view(np.uint32)) and it.adapter_calls == st.adapter_calls


@pytest.mark.parametrize("world", [2, 8])
def test_config4_bunny_grid_at_its_full_film_under_the_native_domain_scheduler(hip, world):
    """BASELINE config 4 at the film of data/bunny.conf:8 (1900 x 1080): the 8-bunny grid, domain d on rank d mod N
    (DomainTracer.h:115-144), through the native Domain scheduler on `world` in-process ranks -- asynchronous ticks and BSP rounds --
    against the oracle's restated DomainTracer and its one-rank image: whole float framebuffer bit for bit, equal ray counts."""
    from gravit_amd.layouts import NORMALS_SMOOTH
    from tests.helpers import oracle_render_domain
    from tests.test_gpu_native import run_native_ranks

    sc = scenes.bunny_grid_scene()
    assert (sc.camera.width, sc.camera.height) == (1900, 1080) and sc.n_inst == 8
    owner = [i % world for i in range(sc.n_inst)]
    ref, st = oracle_render_domain(sc, owner, world, NORMALS_SMOOTH, nthreads=16)
    one, _ = oracle_render(sc, NORMALS_SMOOTH, nthreads=16)
    assert (ref[..., 3] > 0).sum() > 50_000 and np.array_equal(ref[..., :3].view(np.uint32), one[..., :3].view(np.uint32))
    for bsp in (False, True):
        res = run_native_ranks(sc, owner, world, NORMALS_SMOOTH, bsp)
        fb = res[0][0]
        assert np.array_equal(fb[..., :3].view(np.uint32), ref[..., :3].view(np.uint32)) and np.array_equal(fb[..., 3], ref[..., 3])
        assert sum(r[1]["rays_sent"] for r in res.values()) == st.rays_sent and st.rays_sent > 1000
        assert sum(r[1]["rays_closest"] for r in res.values()) == st.rays_closest and sum(r[1]["rays_any"] for r in res.values()) == st.rays_any


def test_benchmark_soup_in_8_tiles_under_the_native_domain_scheduler_at_full_size(hip):
    """The benchmark scene itself -- 10,000,000 triangles, 1920x1080 -- cut into 8 x-y tiles, a tile per rank (8 in-process ranks,
    asynchronous ticks): the composited float framebuffer against the checker's restated DomainTracer, bit for bit, with equal ray counts
    and rays sent -- under the reference's hop-by-hop shuffle rule (the default) and under the opt-in known-miss shortcut (against its
    restatement): on this scene the same image from fewer rays and fewer exchanges."""
    from tests.helpers import oracle_render_domain
    from tests.test_gpu_native import run_native_ranks

    sc = scenes.soup_domains_scene(10_000_000, 8)
    owner = list(range(8))
    out = {}
    for rule, skip in (("strict", 0), ("shortcut", 1)):
        res = run_native_ranks(sc, owner, 8, NORMALS_FLAT, False, opts=(("skip_known", skip),))
        fb = res[0][0]
        ref, st = oracle_render_domain(sc, owner, 8, NORMALS_FLAT, nthreads=16, rule=rule)
        assert (ref[..., 3] > 0).sum() > 1_000_000
        assert np.array_equal(fb[..., :3].view(np.uint32), ref[..., :3].view(np.uint32)) and np.array_equal(fb[..., 3], ref[..., 3])
        assert sum(r[1]["rays_sent"] for r in res.values()) == st.rays_sent and st.rays_sent > 10_000
        assert sum(r[1]["rays_closest"] for r in res.values()) == st.rays_closest and sum(r[1]["rays_any"] for r in res.values()) == st.rays_any
        out[rule] = (ref, st, max(r[1]["rounds"] for r in res.values()))
    assert out["shortcut"][2] <= 6 < out["strict"][2]
    assert np.array_equal(out["strict"][0].view(np.uint32), out["shortcut"][0].view(np.uint32))
    st0, st = out["strict"][1], out["shortcut"][1]
    assert st0.rays_sent > st.rays_sent and st0.rays_closest > st.rays_closest and st0.rounds > st.rounds
