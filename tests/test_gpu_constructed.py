"""GPU parity on constructed scenes (tests/constructed_scenes.py): the HIP path against the CPU
oracle at the sizes where the ordering and binning kernels change behaviour, and with depth ties.

The scenes' counts are exact by construction and checked against the oracle on the CPU
(tests/test_constructed_scenes.py).  Every case here runs in the exact numerics mode and asserts,
with no pixel and no Gaussian left out:
  - image and radii bit-equal to the oracle;
  - every forward intermediate equal (num_rendered, tiles_touched, the tile-sorted list, ranges,
    splat attributes, n_contrib, final_T): the list and the ranges are what sees a wrong tie order
    or a misplaced range edge;
  - every gradient at the 1e-5 contract of tests/test_gpu_parity.py (|gpu - oracle| <= 1e-5 |oracle|
    + 1e-5 max|oracle|), the conic -> covariance chain gradients also within the fp32-order noise
    bound (_check_chain_noise).
dL/dimage is gs_scenes.dl_dimage(..., scale=1.0).  "ratio" in the docstrings is the largest
|gpu - oracle| / bound over all gradients and cases of the test, measured on MI355X."""
import types

import numpy as np
import pytest
import torch

import constructed_scenes as cs_mod
import gs_scenes
from constructed_scenes import cached, oracle_forward
from gpu_checks import exact_mode  # noqa: F401
from test_gpu_parity import RTOL, _check_backward, _check_chain_noise, _check_forward_exact, _gpu_run, _oracle_scene

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("exact_mode")]


_GRADS = (("means2D", "dmeans2D"), ("opacities", "dopacity"), ("means3D", "dmeans3D"), ("shs", "dsh"),
          ("scales", "dscales"), ("rotations", "drotations"))


def _worst_ratio(leaves, gr):
    worst, where = 0.0, ""
    for k, o in _GRADS:
        gpu = leaves[k].grad.detach().cpu().numpy().astype(np.float64)
        ref = np.asarray(gr[o], np.float64)
        tol = RTOL * np.abs(ref) + RTOL * max(np.abs(ref).max(), 1e-30)
        r = float((np.abs(gpu - ref) / tol).max())
        if r > worst:
            worst, where = r, o
    return worst, where


def _parity(oracle, device, cs, dpix_seed=1):
    """The whole comparison for one constructed scene; returns the largest gradient / bound ratio."""
    cam, sc, bg = cs.cam, cs.scene, cs.bg
    W, H = cam.image_width, cam.image_height
    ofw = oracle_forward(oracle, cs)
    assert ofw["num_rendered"] == cs.I and int((ofw["tiles_touched"] > 0).sum()) == cs.V
    _check_forward_exact(ofw, cam, sc, device)
    dpix = gs_scenes.dl_dimage(H, W, seed=dpix_seed, scale=1.0).numpy()
    img, radii, leaves = _gpu_run(cam, sc, device, bg, dpix)
    np.testing.assert_array_equal(img.detach().cpu().numpy(), ofw["color"])
    np.testing.assert_array_equal(radii.cpu().numpy(), ofw["radii"])
    osc = _oracle_scene(oracle, cam, sc, bg)
    gr = oracle.backward(osc, dpix)
    ratio, where = _worst_ratio(leaves, gr)
    print(f"\n[constructed {cs.name}] I={cs.I} V={cs.V} P={cs.P}: worst gradient / bound {ratio:.3f} ({where})")
    _check_backward(gr, leaves)
    _check_chain_noise(leaves, gr, oracle.backward_f32_acc(osc, dpix))
    absent = torch.as_tensor(cs.props["absent"], device=device)
    for k in leaves:  # a Gaussian without an instance has exactly zero gradients
        assert not leaves[k].grad[absent].any(), k
    return ratio


@pytest.mark.parametrize("N", cs_mod.EXACT_SIZES)
def test_exact_instance_counts(oracle, device, N):
    """I = V = N on and around the sort tile (SORT_TILE = 2048 keys, 4 waves x 512; n < 64), the
    look-back scan tile (LB_TILE = 2048), the duplicate block (DUP_SLOTS = 2048 slots: at
    N >= 2048 a block of 2048 one-slot segments, s_seg_base / s_seg_gid exactly full), the k_ranges
    workgroup (1024 instances) and the record-sum wave (64 ranks, 64 one-record owners per chunk).
    Depths cycle over three values (ties everywhere), index order is shuffled, N // 3 absent
    Gaussians are interleaved.  MI355X: ratio 0.19 (dscales, N = 1)."""
    _parity(oracle, device, cached(cs_mod.exact_size, N), dpix_seed=N)


@pytest.mark.parametrize("P", cs_mod.EXACT_TOTALS)
def test_exact_gaussian_counts(oracle, device, P):
    """P itself on and around the sort tile (SORT_TILE = 2048): the first depth-sort pass reads n = P
    keys in index order and drops the quarter of them that have no instance (DEPTH_DROP), the
    later passes sort the V = P - P // 4 survivors.  MI355X: ratio 0.02 (dopacity)."""
    cs = cached(cs_mod.exact_total, P)
    assert cs.P == P
    _parity(oracle, device, cs, dpix_seed=P)


def test_range_edge_on_ranges_workgroup_edge(oracle, device):
    """256 tiles x 8 instances, I = 2048: a range edge on every second k_ranges lane (4 instances per
    lane) and one exactly on the workgroup edge (instance 1024).  MI355X: ratio 0.014 (dmeans3D)."""
    _parity(oracle, device, cached(cs_mod.exact_size, 2048, 256, 256))


@pytest.mark.parametrize("W,H", [(203, 117), (256, 256), (272, 256)])
def test_one_instance_per_tile(oracle, device, W, H):
    """Every instance its own range (k_ranges: both edges of every instance).  256 x 256 has 256
    tiles = 8 tile bits, a single 8-bit tile-sort pass; 272 x 256 has 272 tiles = 9 bits, two
    passes with a narrower first digit (RADIX_BITS = 8).  MI355X: ratio 0.014 (dscales)."""
    _parity(oracle, device, cached(cs_mod.one_per_tile, W, H))


def test_ties_across_sort_tiles(oracle, device):
    """5200 Gaussians with one depth bit pattern, as clone pairs whose colour order decides the image
    (the CPU test shows the reversed tie order renders another image): the LSD radix sort must stay
    stable across the three 2048-key sort tiles (SORT_TILE) of both the depth sort and the tile
    sort for the (tile, depth, index) order DESIGN.md promises.  MI355X: ratio 0.057 (dscales)."""
    _parity(oracle, device, cached(cs_mod.tie_clones))


def test_depth_digit_extremes(oracle, device):
    """Depth keys whose three low bytes come from {00, 01, 7F, 80, FE, FF}: radix digit bins 0 and
    255 (RADIX = 256) populated in every depth-sort pass, every key twice.  MI355X: ratio 0.017 (dmeans3D)."""
    _parity(oracle, device, cached(cs_mod.digit_extremes))


@pytest.mark.parametrize("L", cs_mod.HOT_LENGTHS)
def test_hot_tile_list_lengths(oracle, device, L):
    """One tile with a list of L entries that all contribute (n_eff = L), every other tile empty:
    L on and around the 64 entries staged per round of k_render_fwd_q (FWDQ_NB) and
    k_render_bwd_tw (batches of 64); one range over the whole list.  MI355X: ratio 0.28 (dscales, L = 255)."""
    _parity(oracle, device, cached(cs_mod.hot_tile, L), dpix_seed=L)


def test_two_hot_tiles_last_tile_of_grid(oracle, device):
    """L = 257 in the centre tile and in the last tile of the grid (the last range ends at I).
    MI355X: ratio 0.25 (dmeans3D)."""
    _parity(oracle, device, cached(cs_mod.hot_tile, 257, True))


@pytest.mark.parametrize("n_eff,variant", [(n, "single") for n in cs_mod.STOP_N_EFF] +
                         [(65, "tail_here"), (129, "tail_elsewhere")])
def test_stop_on_round_edge(oracle, device, n_eff, variant):
    """Compositing stops exactly n_eff entries into a list more than twice as long, n_eff on and
    around the 64-entry rounds of the render kernels: the backward walks n_eff entries, tile_cut /
    cut_max (k_tile_order) end the records there, and k_sum_records must neither read nor sum the
    records past the cut (whole 64-record chunks lie behind every tile's cut; they are never
    written, so reading one would add stale memory to a gradient).  "tail_elsewhere": the long
    tail sits in another tile than the one holding cut_max.  MI355X: ratio 0.17 (dscales, 63 single)."""
    _parity(oracle, device, cached(cs_mod.stop_edge, n_eff, variant), dpix_seed=n_eff)


@pytest.mark.parametrize("kind", ["straddle", "chunk_start", "pair"])
def test_one_owner_many_records(oracle, device, kind):
    """A full-screen Gaussian at 320 x 240: 300 instances in 15 row segments of 20.  "straddle": its
    records are slots [1898, 2198), so slot 2048 (DUP_SLOTS: the k_duplicate_lb block edge, where a
    segment starts before the block's k0; also the sort-tile edge) falls inside a row segment.
    "chunk_start": its run starts on slot 320, exactly on a 64-record chunk base of k_sum_records,
    and spans five chunks.  "pair": two such Gaussians at one depth.  MI355X: ratio 0.057 (dopacity, pair)."""
    _parity(oracle, device, cached(cs_mod.big_owner, kind))


@pytest.mark.parametrize("P", [cs_mod.LB_MAX_P, cs_mod.LB_MAX_P + 1])
def test_ordering_path_switch(oracle, device, P):
    """P = 1,048,576 is the last size of the look-back ordering path (lb_tiles(P) = 512 =
    LB_STATIC_MAX: fwd_order / fwd_scan), 1,048,577 the first of the large-scene path (tile counts
    carried through the depth sort, k_scan_reduce / k_scan_down).  All but 2049 Gaussians are
    behind the camera; the 2049 are scattered through the index range, with ties.
    MI355X: ratio 0.022 (dscales)."""
    _parity(oracle, device, cached(cs_mod.path_switch, P))


def test_prepared_views_with_different_exact_counts(oracle, device):
    """Two prepared views (prepare_views: one preprocess and one ordering launch set for both) whose
    counts sit on either side of SORT_TILE / DUP_SLOTS: I = V = 2049 in view A, 2048 in view B.
    Each view is bit-equal to its single-view call and to the oracle (image, radii), with the
    gradients bit-equal to the single-view call and at the contract against the oracle.
    MI355X: ratio 0.022 (dscales)."""
    from diff_gaussian_rasterization import GaussianRasterizer, prepare_views

    cs, cam_b, pb = cached(cs_mod.two_views)
    sc, bg = cs.scene, cs.bg
    cams = [cs.cam, cam_b]
    W, H = cs.cam.image_width, cs.cam.image_height
    dpix = gs_scenes.dl_dimage(H, W, seed=3, scale=1.0).numpy()
    d = sc.to(device)
    rasts = [GaussianRasterizer(gs_scenes.raster_settings_for(c, 0, bg=torch.tensor(bg, device=device), device=device))
             for c in cams]
    names = ("means3D", "shs", "opacities", "scales", "rotations")
    lv = {k: getattr(d, k).clone().requires_grad_(True) for k in names}
    pre = prepare_views(rasts, lv["means3D"], lv["opacities"], shs=lv["shs"], scales=lv["scales"],
                        rotations=lv["rotations"])
    for v, (cam, r, p, I) in enumerate(zip(cams, rasts, pre, (cs.I, pb["I"]))):
        m2 = torch.zeros_like(lv["means3D"], requires_grad=True)
        img, radii = r(means3D=lv["means3D"], means2D=m2, opacities=lv["opacities"], shs=lv["shs"],
                       scales=lv["scales"], rotations=lv["rotations"], prepared=p)
        (img * torch.tensor(dpix, device=device)).sum().backward()
        torch.cuda.synchronize()
        got = {k: types.SimpleNamespace(grad=t.grad.clone()) for k, t in lv.items()}
        got["means2D"] = types.SimpleNamespace(grad=m2.grad.clone())
        for t in lv.values():
            t.grad = None
        osc = _oracle_scene(oracle, cam, sc, bg)
        ofw = oracle.forward(osc, intermediates=True)
        ofw["bg"] = bg
        assert ofw["num_rendered"] == I
        np.testing.assert_array_equal(img.detach().cpu().numpy(), ofw["color"])
        np.testing.assert_array_equal(radii.cpu().numpy(), ofw["radii"])
        _check_forward_exact(ofw, cam, sc, device)
        img1, radii1, single = _gpu_run(cam, sc, device, bg, dpix)
        assert torch.equal(img1, img) and torch.equal(radii1, radii)
        for k in got:
            assert torch.equal(single[k].grad, got[k].grad), (v, k)
        gr = oracle.backward(osc, dpix)
        ratio, where = _worst_ratio(got, gr)
        print(f"\n[constructed two_views {'AB'[v]}] I={I}: worst gradient / bound {ratio:.3f} ({where})")
        _check_backward(gr, got)
        _check_chain_noise(got, gr, oracle.backward_f32_acc(osc, dpix))


# ------------------------------------------------------------------------------------------
# grids above 1080p: the tile sort's later pass plans
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,bits", cs_mod.LARGE_GRIDS)
def test_one_instance_per_tile_above_1080p(oracle, device, W, H, bits):
    """test_one_instance_per_tile continued past 1080p (8,160 tiles, 13 tile bits, 6 + 7): 8,256 tiles
    = 14 bits sorted as 7 + 7, 16,512 = 15 bits as 7 + 8, 32,896 and 65,536 (exactly 2^16, no ragged
    edge) = 16 bits as 8 + 8, and 65,792 = 17 bits, the first three-pass tile sort (5 + 6 + 6), whose
    sorted list ends in the other ping-pong buffer (bin_layout's host-side parity against
    radix_sort_pairs' own), with k_duplicate_lb counting the 5-bit first digit.  k_ranges,
    k_tile_order and the scheduling words run over up to 8 times the tiles of 1080p.
    MI355X: ratio 0.016 (dscales, 4107 x 2037)."""
    _parity(oracle, device, cached(cs_mod.one_per_tile, W, H))


def test_ties_through_three_tile_sort_passes(oracle, device):
    """80,000 Gaussians with one depth bit pattern on the 17-bit grid (4107 x 4085), as clone pairs in
    the first 40,000 tiles: the tile sort alone orders the list, so the (tile, index) order -- and the
    image, which the clones' colour order decides -- needs all three passes (5 + 6 + 6) to be
    stable across 40 sort tiles.  MI355X: ratio 0.013 (dscales)."""
    _parity(oracle, device, cached(cs_mod.tie_clones, 40000, *cs_mod.GRID17))


def test_owners_past_65535_records_per_splat_duplicate(oracle, device):
    """few_big on the 17-bit grid: three full-screen Gaussians of 65,792 instances each (two at one
    depth) and five one-tile ones in tiles 0, 256, 65535, 65536, 65791; P = 12, I = 197,381, so
    dup_balanced is false and the per-splat k_duplicate writes owners' runs longer than 65,535
    records, followed by the three-pass tile sort without the duplicate's first-digit counts.
    MI355X: ratio 0.030 (dmeans3D)."""
    _parity(oracle, device, cached(cs_mod.few_big))


def test_owner_past_65535_records_lookback_duplicate(oracle, device):
    """owner_among_many on the 17-bit grid: a one-tile Gaussian in every tile and one full-screen
    Gaussian among them; P = 66,793, I = 131,584 (balanced), so k_duplicate_lb runs and the one
    owner's 65,792 records cross 33 duplicate blocks (each finds the row segment that began before
    its first slot), with the first digit counted under the 5-bit mask.
    MI355X: ratio 0.014 (dmeans3D)."""
    _parity(oracle, device, cached(cs_mod.owner_among_many))


def test_prepared_views_three_pass_batched_sort(oracle, device):
    """Two prepared views of the 4107 x 4085 one_per_tile scene (17 tile bits): the batched tile sort
    (views = 2, every array one view stride apart) goes through three passes and both views' lists
    end in the second ping-pong buffer.  Camera B is the identity camera moved right by 16 * 3 / fx:
    every Gaussian (all at z = 3) moves one whole tile to the left, tile column 0 leaves the image,
    I = 65,792 in A and 65,536 = 2^16 in B.  Each view is bit-equal to its single-view call (image,
    radii, gradients) and to the oracle (image, radii, every intermediate), the gradients at the
    contract against the oracle.  MI355X: ratio 0.014 (dscales, view B)."""
    from diff_gaussian_rasterization import GaussianRasterizer, prepare_views

    W, H = cs_mod.GRID17
    cs = cached(cs_mod.one_per_tile, W, H)
    gx, gy = cs_mod.grid(W, H)
    sc, bg = cs.scene, cs.bg
    fx = W / (2.0 * np.tan(cs.cam.FoVx / 2))
    cam_b = gs_scenes.make_camera(np.eye(3), np.array([-cs_mod.TILE * 3.0 / fx, 0.0, 0.0]), W, H)
    cams = [cs.cam, cam_b]
    dpix = gs_scenes.dl_dimage(H, W, seed=5, scale=1.0).numpy()
    d = sc.to(device)
    rasts = [GaussianRasterizer(gs_scenes.raster_settings_for(c, 0, bg=torch.tensor(bg, device=device), device=device))
             for c in cams]
    names = ("means3D", "shs", "opacities", "scales", "rotations")
    lv = {k: getattr(d, k).clone().requires_grad_(True) for k in names}
    pre = prepare_views(rasts, lv["means3D"], lv["opacities"], shs=lv["shs"], scales=lv["scales"],
                        rotations=lv["rotations"])
    for v, (cam, r, p, I) in enumerate(zip(cams, rasts, pre, (gx * gy, (gx - 1) * gy))):
        m2 = torch.zeros_like(lv["means3D"], requires_grad=True)
        img, radii = r(means3D=lv["means3D"], means2D=m2, opacities=lv["opacities"], shs=lv["shs"],
                       scales=lv["scales"], rotations=lv["rotations"], prepared=p)
        (img * torch.tensor(dpix, device=device)).sum().backward()
        torch.cuda.synchronize()
        got = {k: types.SimpleNamespace(grad=t.grad.clone()) for k, t in lv.items()}
        got["means2D"] = types.SimpleNamespace(grad=m2.grad.clone())
        for t in lv.values():
            t.grad = None
        osc = _oracle_scene(oracle, cam, sc, bg)
        ofw = oracle.forward(osc, intermediates=True)
        ofw["bg"] = bg
        assert ofw["num_rendered"] == I
        assert (ofw["ranges"][:, 1].astype(np.int64) - ofw["ranges"][:, 0] ==
                (np.arange(gx * gy) % gx < gx - v).astype(np.int64)).all()
        np.testing.assert_array_equal(img.detach().cpu().numpy(), ofw["color"])
        np.testing.assert_array_equal(radii.cpu().numpy(), ofw["radii"])
        _check_forward_exact(ofw, cam, sc, device)
        del ofw
        img1, radii1, single = _gpu_run(cam, sc, device, bg, dpix)
        assert torch.equal(img1, img) and torch.equal(radii1, radii)
        for k in got:
            assert torch.equal(single[k].grad, got[k].grad), (v, k)
        del img1, single, img
        gr = oracle.backward(osc, dpix)
        ratio, where = _worst_ratio(got, gr)
        print(f"\n[constructed three_pass_views {'AB'[v]}] I={I}: worst gradient / bound {ratio:.3f} ({where})")
        _check_backward(gr, got)
        _check_chain_noise(got, gr, oracle.backward_f32_acc(osc, dpix))


# ------------------------------------------------------------------------------------------
# distCUDA2 at its own boundaries
# ------------------------------------------------------------------------------------------
def _knn_check(oracle, device, pts):
    from simple_knn._C import distCUDA2

    pts = np.ascontiguousarray(pts, np.float32)
    got = distCUDA2(torch.from_numpy(pts).to(device)).cpu().numpy()
    ref = oracle.knn_mean_dist2(pts)
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)
    return got


@pytest.mark.parametrize("P", [31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049])
def test_knn_box_and_sort_tile_sizes(oracle, device, P):
    """P on and around the box (KNN_BOX = 32 points), the super-box (KNN_SUPER = 1024) and the
    sort tile (SORT_TILE = 2048: P is the Morton sort's n), same cloud as test_knn_matches_oracle."""
    g = torch.Generator().manual_seed(P)
    pts = torch.randn((P, 3), generator=g) * torch.tensor([3.0, 1.0, 0.5])
    got = _knn_check(oracle, device, pts.numpy())
    assert np.isfinite(got).all() and (got > 0).all()


def _knn_shapes():
    P = 1025
    rng = np.random.default_rng(4)
    base = (rng.normal(size=(P, 3)) * np.array([3.0, 1.0, 0.5])).astype(np.float32)
    dup = np.concatenate([base[:513], base[:512]])
    planar = base.copy()
    planar[:, 1] = 0.25
    line = np.outer(rng.normal(size=P), np.array([1.0, -2.0, 0.5])).astype(np.float32)
    cluster = (rng.normal(size=(P, 3)) * 1e-3).astype(np.float32)
    cluster[:4] = np.array([[1e3, 0, 0], [0, -1e3, 0], [0, 0, 1e3], [-1e3, 1e3, 0]], np.float32)
    return {"duplicated": dup, "identical": np.full((P, 3), 1.5, np.float32), "planar": planar, "collinear": line,
            "cluster_outliers": cluster}


@pytest.mark.parametrize("shape", ["duplicated", "identical", "planar", "collinear", "cluster_outliers"])
def test_knn_degenerate_clouds(oracle, device, shape):
    """P = 1025 (one past KNN_SUPER): every point duplicated (nearest distance 0; the last point
    once), all points identical (every Morton code equal, ext == 0 on all axes in k_knn_morton, all
    distances 0), a planar cloud (ext == 0 on one axis), a collinear cloud, and a tight cluster plus
    four far outliers (nearly all Morton codes collide in one cell)."""
    pts = _knn_shapes()[shape]
    got = _knn_check(oracle, device, pts)
    if shape == "identical":
        assert (got == 0).all()
    if shape == "duplicated":
        assert (got[:512] == got[513:]).all()


@pytest.mark.parametrize("P", [1, 2, 3])
def test_knn_fewer_than_four_points(oracle, device, P):
    """Fewer than 3 neighbours: a missing neighbour counts as FLT_MAX (the 3-best list's initial
    value, as upstream), so P = 3 returns (d0 + d1 + FLT_MAX) / 3 = FLT_MAX / 3 = 1.134e38 (finite) and
    P = 1, 2 overflow to +inf.  The oracle restates exactly that; the values are compared bit for
    bit (inf == inf)."""
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]], np.float32)[:P]
    got = _knn_check(oracle, device, pts)
    ref = oracle.knn_mean_dist2(pts)
    np.testing.assert_array_equal(got, ref)
    if P == 3:
        assert np.isfinite(got).all() and (got == np.float32(np.finfo(np.float32).max) / np.float32(3.0)).all()
    else:
        assert np.isposinf(got).all()
