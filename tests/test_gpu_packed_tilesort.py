"""GPU tests of the packed two-pass tile sort (csrc/gs_forward.hip tile_sort_packed_views): one word
per instance after the first pass, no key output from the second, tile ranges from the second
pass's histogram.  tests/test_packed_tilesort_cpu.py restates the algorithm.

The packed path runs for two-pass grids (9 .. 16 tile bits) when the buffer's instance capacity is
at least 2^fb sort chunks (fb: the first digit's width), so the small scenes here reach it through
a bounded forward with a capacity above their count.  gs_debug_set_tile_sort_packed switches
between the two paths in one process and gs_debug_tile_sort_packed_count tells which one ran.
Every comparison is bit-exact: the tile-sorted list and the ranges against the (key, slot) pair
path and the CPU oracle, image and gradients between the two paths."""
import numpy as np
import pytest
import torch

import constructed_scenes as cs_mod
import gs_scenes
from constructed_scenes import cached, oracle_forward
from gpu_checks import lib as _lib
from test_gpu_parity import _oracle_scene

pytestmark = pytest.mark.gpu

SORT_TILE = 2048


def first_bits(tiles):
    """(tile bits, first digit's width) of the tile sort: gs_sortscan.h radix_first_bits."""
    bits = max(1, int(tiles - 1).bit_length())
    passes = (bits + 7) // 8
    width = (bits + passes - 1) // passes
    return bits, bits if bits <= width else bits - (passes - 1) * width


def packed_capacity(W, H):
    """the smallest capacity at which the packed path runs for a W x H image"""
    gx, gy = cs_mod.grid(W, H)
    return SORT_TILE << first_bits(gx * gy)[1]


@pytest.fixture(autouse=True)
def exact_mode():
    prev = _lib().gs_set_exact_exp(1)
    yield
    _lib().gs_set_exact_exp(prev)
    _lib().gs_debug_set_tile_sort_packed(1)


def _on_both_paths(fn):
    """fn() with the packed path on, then off: (packed result, pair result, packed binnings of each)"""
    lib = _lib()
    n0 = lib.gs_debug_tile_sort_packed_count()
    lib.gs_debug_set_tile_sort_packed(1)
    a = fn()
    torch.cuda.synchronize()
    n1 = lib.gs_debug_tile_sort_packed_count()
    lib.gs_debug_set_tile_sort_packed(0)
    try:
        b = fn()
        torch.cuda.synchronize()
    finally:
        lib.gs_debug_set_tile_sort_packed(1)
    return a, b, n1 - n0, lib.gs_debug_tile_sort_packed_count() - n1


def _launched():
    lib = _lib()
    import ctypes

    n = lib.gs_debug_launched_kernels(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    lib.gs_debug_launched_kernels(buf, n + 1)
    return buf.value.decode().split()


def _lists(cam, sc, bg, device, cap):
    """(count, tile-sorted Gaussian ids [cap], ranges, image) of a forward with binning capacity `cap` (None: the
    two-call forward, sized for its count)"""
    from diff_gaussian_rasterization import _C

    s = gs_scenes.raster_settings_for(cam, sc.sh_degree, bg=torch.tensor(bg, device=device), device=device)
    d = sc.to(device)
    e = torch.Tensor([])
    num, color, radii, geom, binb, imgb = _C.rasterize_gaussians(
        s.bg, d.means3D, e, d.opacities, d.scales, d.rotations, s.scale_modifier, e, s.viewmatrix, s.projmatrix,
        s.tanfovx, s.tanfovy, s.image_height, s.image_width, d.shs, sc.sh_degree, s.campos, False, False,
        capacity=cap)
    ex = _C.debug_export(sc.P, cam.image_width, cam.image_height, num, geom, binb, imgb, device)
    torch.cuda.synchronize()
    return (ex["point_list"].cpu().numpy().astype(np.uint32), ex["ranges"].cpu().numpy().astype(np.uint32),
            color.cpu().numpy())


def _fwd_bwd(cam, sc, bg, device, cap, dpix):
    from diff_gaussian_rasterization import GaussianRasterizer

    rast = GaussianRasterizer(gs_scenes.raster_settings_for(cam, sc.sh_degree, bg=torch.tensor(bg, device=device),
                                                            device=device))
    d = sc.to(device)
    p = [t.clone().requires_grad_(True) for t in (d.means3D, d.shs, d.opacities, d.scales, d.rotations)]
    m2 = torch.zeros_like(p[0], requires_grad=True)
    img, radii = rast(means3D=p[0], means2D=m2, opacities=p[2], shs=p[1], scales=p[3], rotations=p[4],
                      binning_capacity=cap)
    img.backward(dpix)
    torch.cuda.synchronize()
    return [img.detach(), radii, m2.grad] + [t.grad for t in p]


def _check_scene(device, cam, sc, bg, want_list, want_ranges, cap, expect_packed=True):
    """Both paths at capacity `cap` against the expected list / ranges; image and gradients between the paths."""
    I = len(want_list)
    a, b, na, nb = _on_both_paths(lambda: _lists(cam, sc, bg, device, cap))
    assert (na, nb) == (1 if expect_packed else 0, 0)
    for got in (a, b):
        np.testing.assert_array_equal(got[0][:I], want_list)
        assert (got[0][I:] == 0xFFFFFFFF).all()  # past the count: not written by the forward
        np.testing.assert_array_equal(got[1], want_ranges)
    np.testing.assert_array_equal(a[2], b[2])
    W, H = cam.image_width, cam.image_height
    dpix = gs_scenes.dl_dimage(H, W, seed=2, scale=1.0).to(device)
    ga, gb, na, nb = _on_both_paths(lambda: _fwd_bwd(cam, sc, bg, device, cap, dpix))
    assert (na, nb) == (1 if expect_packed else 0, 0)
    for k, (x, y) in enumerate(zip(ga, gb)):
        assert torch.equal(x, y), k
    if expect_packed:
        assert any("k_ranges_packed" in k for k in _launched())


# ------------------------------------------------------------------------------------------
# both paths, and the oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(256, 256), (272, 256), (640, 400)])
def test_random_scene_lists_equal_pair_path_and_oracle(oracle, device, W, H):
    """A few thousand Gaussians.  256 x 256 is 8 tile bits, one pass: the pair path whatever the switch
    says.  272 x 256 is 9 bits (4 + 5), 640 x 400 is 1000 tiles = 10 bits (5 + 5): packed."""
    cam = gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(3000, 3, cam=cam, seed=W)
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    fw = oracle.forward(_oracle_scene(oracle, cam, sc, bg), intermediates=True)
    two_pass = first_bits(cs_mod.grid(W, H)[0] * cs_mod.grid(W, H)[1])[0] > 8
    cap = max(packed_capacity(W, H), fw["num_rendered"] + 1)
    _check_scene(device, cam, sc, bg, fw["point_list"], fw["ranges"], cap, expect_packed=two_pass)


def region_totals():
    """272 x 256: 272 tiles, 9 tile bits sorted as 4 + 5, so low digit l = tile % 16 and its region of
    the padded first-pass output holds the instances of tiles l, l + 16, ..., 17 of them.  Region totals
    of exactly 2048 and 2049 (a full sort tile; one word into the next), 2047, 1 and 4097, the other
    eleven digits empty; depths cycle over three values (ties), index order shuffled."""
    b = cs_mod.Builder(272, 256, seed=272, bg=(0.1, 0.2, 0.3))
    for l, cnt in ((0, 2048), (1, 2049), (2, 2047), (7, 1), (15, 4097)):
        for k in range(cnt):
            b.add_tile(l + 16 * (k % 17), cs_mod.TIE_DEPTHS[(k // 17) % 3], opacity=float(b.rng.uniform(0.05, 0.5)))
    return b.build("region_totals_272x256", shuffle=True, n_absent=1000)


def test_region_totals_on_the_sort_tile(oracle, device):
    cs = cached(region_totals)
    assert cs.I == 2048 + 2049 + 2047 + 1 + 4097
    fw = oracle_forward(oracle, cs)
    np.testing.assert_array_equal(fw["point_list"], cs.point_list)
    _check_scene(device, cs.cam, cs.scene, cs.bg, fw["point_list"], fw["ranges"], packed_capacity(272, 256))


@pytest.mark.parametrize("W,H,bits", [(700, 460, 11), (1040, 1024, 13), (2059, 1013, 14), (2059, 2037, 15),
                                      (4096, 4096, 16)])
def test_one_instance_per_tile(oracle, device, W, H, bits):
    """Every instance its own range, every tile of the grid non-empty: 11 bits (5 + 6), 13 (6 + 7),
    14 (7 + 7), 15 (7 + 8) and 16 (8 + 8, exactly 2^16 tiles).  The expected list and ranges are the
    construction's (tests/test_constructed_scenes.py holds them against the oracle); up to 1080p the
    oracle's own are compared too."""
    cs = cached(cs_mod.one_per_tile, W, H)
    gx, gy = cs_mod.grid(W, H)
    assert first_bits(gx * gy)[0] == bits and cs.I == gx * gy
    if W * H <= cs_mod.CACHE_MAX_PIXELS:
        fw = oracle_forward(oracle, cs)
        np.testing.assert_array_equal(fw["point_list"], cs.point_list)
        np.testing.assert_array_equal(fw["ranges"], cs.ranges)
    _check_scene(device, cs.cam, cs.scene, cs.bg, cs.point_list, cs.ranges, packed_capacity(W, H))


# ------------------------------------------------------------------------------------------
# bounded forwards
# ------------------------------------------------------------------------------------------
BW, BH = 320, 240  # 300 tiles: 9 bits (4 + 5), packed from 32,768 instances


def _ball(device, seed=5):
    return gs_scenes.random_gaussians(100_000, 3, seed=seed, ball_radius=2.0)


def test_capacity_above_at_and_below_the_count(device):
    from diff_gaussian_rasterization import bounded_status, last_num_rendered

    sc = _ball(device)
    cam = gs_scenes.circle_cameras(1, 6.0, BW, BH)[0]
    bg = np.zeros(3, np.float32)
    dpix = gs_scenes.dl_dimage(BH, BW, seed=4).to(device)
    ref = _fwd_bwd(cam, sc, bg, device, None, dpix)
    n = last_num_rendered()
    below = max(n // 3, packed_capacity(BW, BH))  # still packed
    assert below < n
    for cap in (int(n * 1.37) + 5, n):
        a, b, na, nb = _on_both_paths(lambda: _fwd_bwd(cam, sc, bg, device, cap, dpix))
        assert (na, nb) == (1, 0)
        for k, (r, x, y) in enumerate(zip(ref, a, b)):
            assert torch.equal(r, x) and torch.equal(r, y), (cap, k)
    assert bounded_status() == (0, 0)
    # fewer than the instances: placeholders in bounds, nothing composited, the sticky status raises
    n0 = _lib().gs_debug_tile_sort_packed_count()
    got = _fwd_bwd(cam, sc, bg, device, below, dpix)
    assert _lib().gs_debug_tile_sort_packed_count() == n0 + 1
    assert torch.equal(got[0], torch.zeros_like(got[0])) and torch.equal(got[1], ref[1])
    for g in got[2:]:
        assert torch.isfinite(g).all() and float(g.abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="binning capacity"):
        bounded_status()
    assert bounded_status() == (0, 0)
    again = _fwd_bwd(cam, sc, bg, device, n, dpix)
    for r, x in zip(ref, again):
        assert torch.equal(r, x)


def _views_step(device, sc, cams, dpix, cap):
    """prepare_views (batched binning of the views) + renders + backwards; [images, summed gradients]"""
    from diff_gaussian_rasterization import GaussianRasterizer, prepare_views

    rasts = [GaussianRasterizer(gs_scenes.raster_settings_for(c, 3, device=device)) for c in cams]
    d = sc.to(device)
    p = [t.clone().requires_grad_(True) for t in (d.means3D, d.shs, d.opacities, d.scales, d.rotations)]
    pres = prepare_views(rasts, p[0], p[2], shs=p[1], scales=p[3], rotations=p[4], binning_capacity=cap)
    imgs = []
    for r, pre, dp in zip(rasts, pres, dpix):
        img, _ = r(means3D=p[0], means2D=torch.zeros_like(p[0], requires_grad=True), opacities=p[2], shs=p[1],
                   scales=p[3], rotations=p[4], prepared=pre)
        img.backward(dp)
        imgs.append(img.detach())
    torch.cuda.synchronize()
    return imgs + [t.grad for t in p]


def test_two_prepared_views_with_unequal_counts(device):
    """One batched binning of two views whose counts differ (both below the shared capacity)."""
    from diff_gaussian_rasterization import last_num_rendered

    sc = _ball(device, seed=9)
    cams = [gs_scenes.circle_cameras(1, 6.0, BW, BH)[0], gs_scenes.circle_cameras(1, 9.0, BW, BH)[0]]
    dpix = [gs_scenes.dl_dimage(BH, BW, seed=60 + v).to(device) for v in range(2)]
    counts = []
    for c in cams:
        _fwd_bwd(c, sc, np.zeros(3, np.float32), device, None, dpix[0])
        counts.append(last_num_rendered())
    assert counts[0] != counts[1] and min(counts) >= packed_capacity(BW, BH)
    cap = int(max(counts) * 1.25)
    a, b, na, nb = _on_both_paths(lambda: _views_step(device, sc, cams, dpix, cap))
    assert na >= 1 and nb == 0
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), k


def test_captured_graph_replay_equals_eager(device):
    from diff_gaussian_rasterization import bounded_status, last_num_rendered

    sc = _ball(device, seed=11)
    cam = gs_scenes.circle_cameras(1, 6.0, BW, BH)[0]
    bg = np.zeros(3, np.float32)
    dpix = gs_scenes.dl_dimage(BH, BW, seed=8).to(device)
    ref = _fwd_bwd(cam, sc, bg, device, None, dpix)
    cap = int(last_num_rendered() * 1.25)
    from diff_gaussian_rasterization import GaussianRasterizer

    rast = GaussianRasterizer(gs_scenes.raster_settings_for(cam, 3, bg=torch.tensor(bg, device=device), device=device))
    d = sc.to(device)
    p = [t.clone().requires_grad_(True) for t in (d.means3D, d.shs, d.opacities, d.scales, d.rotations)]
    m2 = torch.zeros_like(p[0], requires_grad=True)
    out = {}

    def step():  # (autograd.grad: no gradient accumulation into leaves made on another stream)
        img, radii = rast(means3D=p[0], means2D=m2, opacities=p[2], shs=p[1], scales=p[3], rotations=p[4],
                          binning_capacity=cap)
        out["v"] = [img.detach(), radii] + list(torch.autograd.grad(img, [m2] + p, dpix))

    n0 = _lib().gs_debug_tile_sort_packed_count()
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    assert _lib().gs_debug_tile_sort_packed_count() == n0 + 3
    for _ in range(2):
        for t in out["v"]:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, (r, x) in enumerate(zip(ref, out["v"])):
            assert torch.equal(r, x), k
    assert bounded_status() == (0, 0)
    del graph


# ------------------------------------------------------------------------------------------
# the fallback rule
# ------------------------------------------------------------------------------------------
def test_three_pass_grid_takes_the_pair_path(oracle, device):
    """4107 x 4085: 65,792 tiles, 17 tile bits, three passes."""
    W, H = cs_mod.GRID17
    cs = cached(cs_mod.one_per_tile, W, H)
    _check_scene(device, cs.cam, cs.scene, cs.bg, cs.point_list, cs.ranges, 1 << 20, expect_packed=False)


def test_capacity_too_small_for_the_padded_intermediate_takes_the_pair_path(oracle, device):
    """One word below 2^fb sort chunks the padded intermediate no longer fits keys_b | vals_b."""
    cs = cached(region_totals)
    cap = packed_capacity(272, 256)
    for c, packed in ((cap - 1, False), (cap, True)):
        a, b, na, nb = _on_both_paths(lambda: _lists(cs.cam, cs.scene, cs.bg, device, c))
        assert (na, nb) == (int(packed), 0)
        for got in (a, b):
            np.testing.assert_array_equal(got[0][:cs.I], cs.point_list)
            np.testing.assert_array_equal(got[1], cs.ranges)


def test_capacity_that_does_not_fit_the_packed_word_takes_the_pair_path(device):
    """16 tile bits leave 8 high bits beside the slot: a capacity of 2^24 instances or more does not fit
    (hb + sb <= 32 with capacity < 2^sb), one below it does."""
    cs = cached(cs_mod.one_per_tile, 4096, 4096)
    for c, packed in (((1 << 24) - 1, True), (1 << 24, False)):
        a, b, na, nb = _on_both_paths(lambda: _lists(cs.cam, cs.scene, cs.bg, device, c))
        assert (na, nb) == (int(packed), 0)
        for got in (a, b):
            np.testing.assert_array_equal(got[0][:cs.I], cs.point_list)
            np.testing.assert_array_equal(got[1], cs.ranges)
