"""GPU tests of the batched K-view instance-offsets scan (fwd_order with views > 1): the views'
scans run as one k_scan_reduce / k_scan_partials / k_scan_down set (blockIdx.y = view) instead of
one look-back k_scan_lb launch per view, over the tile counts the depth sort's first scatter packs
beside the ids in its value words (up to 1M Gaussians) or carries as a second value stream (above).
The reference is the path that did not change: K plain
single-view calls, which still scan with k_scan_lb.  Every comparison is bit for bit (the offsets
are integers): num_rendered, image, radii, every field of _C.debug_export (tile counts, point
list, ranges, final_T, n_contrib) and, once per test, every gradient after one backward per view.
The helpers follow tests/test_gpu_preprocess_views.py."""
import numpy as np
import pytest
import torch

import constructed_scenes as C
import gs_scenes

pytestmark = pytest.mark.gpu

W, H = 70, 45  # neither a multiple of the 16-pixel tile
DUP_SLOTS = C.DUP_SLOTS


def _cams(K, w=W, h=H):
    return gs_scenes.jittered_cameras(K, w, h, seed=11, max_angle_deg=6.0, max_shift=0.3)


def _scene(P, deg, seed=3, cam=None):
    cam = cam or gs_scenes.identity_camera(W, H)
    return gs_scenes.random_gaussians(P, deg, cam=cam, seed=seed, scale_range=(0.02, 0.3))


def _settings(cams, deg, device):
    return [gs_scenes.raster_settings_for(c, deg, device=device) for c in cams]


def _inputs(sc, device):
    d = sc.to(device)
    return dict(means3D=d.means3D, opacities=d.opacities, shs=d.shs, scales=d.scales, rotations=d.rotations)


def _preprocess(ss, inp, deg, capacity=None):
    """_C.preprocess_views of the K views; capacity: None (eager), one int or one per view (bounded)."""
    from diff_gaussian_rasterization import _C

    e = torch.Tensor([])
    g = lambda k: inp.get(k, e)  # noqa: E731
    s0 = ss[0]
    if capacity is not None and not isinstance(capacity, (list, tuple)):
        capacity = [capacity] * len(ss)
    return _C.preprocess_views([s.bg for s in ss], inp["means3D"], g("colors_precomp"), inp["opacities"],
                               g("scales"), g("rotations"), s0.scale_modifier, g("cov3D_precomp"),
                               [s.viewmatrix for s in ss], [s.projmatrix for s in ss], [s.tanfovx for s in ss],
                               [s.tanfovy for s in ss], [s.image_height for s in ss], [s.image_width for s in ss],
                               g("shs"), deg, [s.campos for s in ss], False, False, None,
                               None if capacity is None else list(capacity))


def _buffers(ss, inp, deg, prepared, capacity=None):
    """Each view's (num_rendered, color, radii, debug_export dict) through _C, plain or prepared."""
    from diff_gaussian_rasterization import _C

    e = torch.Tensor([])
    g = lambda k: inp.get(k, e)  # noqa: E731
    pre = _preprocess(ss, inp, deg, capacity) if prepared else [None] * len(ss)
    out = []
    for s, p in zip(ss, pre):
        num, color, radii, geom, binb, imgb = _C.rasterize_gaussians(
            s.bg, inp["means3D"], g("colors_precomp"), inp["opacities"], g("scales"), g("rotations"), s.scale_modifier,
            g("cov3D_precomp"), s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width,
            g("shs"), deg, s.campos, False, False, prepared=None if p is None else tuple(p))[:6]
        ex = _C.debug_export(inp["means3D"].shape[0], s.image_width, s.image_height, num, geom, binb, imgb,
                             inp["means3D"].device)
        out.append((num, color, radii, ex))
    torch.cuda.synchronize()
    return out


def _autograd(ss, inp, dpix, prepared, capacity=None):
    """Each view's (image, radii, dL/dmeans2D) and the inputs' gradients summed over the views (one
    backward per view, in view order) through GaussianRasterizer, plain or with prepare_views."""
    from diff_gaussian_rasterization import GaussianRasterizer, prepare_views

    leaves = {k: v.clone().requires_grad_(True) for k, v in inp.items()}
    rasts = [GaussianRasterizer(s) for s in ss]
    kw = {k: v for k, v in leaves.items() if k not in ("means3D", "opacities")}
    pre = [None] * len(ss)
    if prepared:
        pre = prepare_views(rasts, leaves["means3D"], leaves["opacities"], binning_capacity=capacity, **kw)
    outs = []
    for r, p, dp in zip(rasts, pre, dpix):
        m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
        img, radii = r(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], prepared=p, **kw)
        img.backward(dp)
        outs.append((img.detach().clone(), radii.clone(), m2.grad.clone()))
    torch.cuda.synchronize()
    return outs, {k: v.grad.clone() for k, v in leaves.items()}


def _plain(ss, inp, deg):
    return _buffers(ss, inp, deg, False)


def _assert_buffers_equal(plain, prep, what=()):
    """A view's own total and offsets show in its ranges (the last range ends at its total) and in
    its point list; views binned together report the largest count as their buffers' layout."""
    for v, ((na, ca, ra, ea), (nb, cb, rb, eb)) in enumerate(zip(plain, prep)):
        at = (*what, v)
        assert nb >= na and (len(plain) > 1 or nb == na), at
        assert torch.equal(ca, cb) and torch.equal(ra, rb), at
        assert na == int(ea["tiles_touched"].sum()), at
        for k in ("tiles_touched", "ranges", "final_T", "n_contrib"):
            assert torch.equal(ea[k], eb[k]), (*at, k)
        assert torch.equal(ea["point_list"], eb["point_list"][:na]), at
        assert int(eb["ranges"].max()) == na, at


def _assert_grads_equal(ss, inp, device, capacity=None):
    dpix = [gs_scenes.dl_dimage(s.image_height, s.image_width, seed=40 + v, scale=1.0).to(device)
            for v, s in enumerate(ss)]
    a_out, a_grad = _autograd(ss, inp, dpix, False)
    b_out, b_grad = _autograd(ss, inp, dpix, True, capacity=capacity)
    for v, (a, b) in enumerate(zip(a_out, b_out)):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), v
    for k in a_grad:
        assert torch.equal(a_grad[k], b_grad[k]), k


SCAN_P = (1, 63, 1023, 1024, 1025, 2049, 5000)


def test_tile_boundaries(device):
    """P below, at and just above one scan tile (SCAN_TILE = 1024 = 256 threads x 4 items), one lone
    row and several workgroups, with 2, 3 and 8 views: the identity view sees (nearly) all P, the
    jittered ones fewer, so the views' scans end inside different tiles.  Gradients once."""
    cams = _cams(8)
    ss8 = _settings(cams, 1, device)
    for P in SCAN_P:
        inp = _inputs(_scene(P, 1, seed=5 + P), device)
        plain = _plain(ss8, inp, 1)  # shared by the three view counts
        if P >= 1023:
            seen = [int((r > 0).sum()) for _, _, r, _ in plain]
            assert seen[0] > 0.9 * P and len(set(seen)) > 1, seen
        for K in (2, 3, 8):
            _assert_buffers_equal(plain[:K], _buffers(ss8[:K], inp, 1, True), (P, K))
        if P == 1025:
            _assert_grads_equal(ss8[:3], inp, device)


def test_counts_differ_per_view(device):
    """One view that looks away (no instances), one with part of the scene behind its near plane
    (V < P) and one that sees everything, in that order and reversed: each view's count, total and
    offsets are its own."""
    P = 2049
    cams = [gs_scenes.look_at_camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), W, H),
            gs_scenes.look_at_camera((0.0, 0.0, 5.0), (0.0, 0.0, 20.0), W, H),
            gs_scenes.identity_camera(W, H)]
    inp = _inputs(_scene(P, 1, seed=13), device)
    for order in (cams, cams[::-1]):
        ss = _settings(order, 1, device)
        plain = _plain(ss, inp, 1)
        seen = sorted(int((r > 0).sum()) for _, _, r, _ in plain)
        assert seen[0] == 0 and 0 < seen[1] < seen[2] and seen[2] > 0.9 * P, seen
        assert sorted(n for n, _, _, _ in plain)[0] == 0
        _assert_buffers_equal(plain, _buffers(ss, inp, 1, True))
    _assert_grads_equal(_settings(cams, 1, device), inp, device)


def test_owners_longer_than_a_duplicate_block(device):
    """800 x 800 (2,500 tiles), P = 64: four screen-filling splats, each with more instances than a
    duplicate block's DUP_SLOTS, among sixty one-tile ones; the average stays below DUP_SLOTS, so the
    balanced duplicate runs and dup_first -- written by the scan's down sweep -- must hand every block
    to its owner: the point list and the ranges show it."""
    b = C.Builder(800, 800, seed=41, bg=(0.0, 0.05, 0.1))
    assert b.tiles == 2500 > DUP_SLOTS
    for j in range(60):
        if j % 15 == 0:
            b.add_all_tiles(2.0 + 0.05 * j, 0.3)
        b.add_tile((41 * j + 7) % b.tiles, 2.0 + 0.05 * j + 0.01, opacity=0.4)
    cs = b.build("views_scan_owners", shuffle=True)
    assert cs.P == 64 and cs.I == 4 * 2500 + 60 and cs.I < DUP_SLOTS * cs.P
    cams = [cs.cam] + gs_scenes.jittered_cameras(2, 800, 800, seed=5, max_angle_deg=1.0, max_shift=0.02)[1:]
    ss = _settings(cams, 0, device)
    inp = _inputs(cs.scene, device)
    plain = _plain(ss, inp, 0)
    n0, _, _, e0 = plain[0]
    assert n0 == cs.I and np.array_equal(e0["point_list"].cpu().numpy(), cs.point_list)
    assert np.array_equal(e0["ranges"].cpu().numpy().reshape(-1, 2), cs.ranges)
    for n, _, _, ex in plain:
        assert int((ex["tiles_touched"] > DUP_SLOTS).sum()) == 4 and n < DUP_SLOTS * cs.P
    _assert_buffers_equal(plain, _buffers(ss, inp, 0, True))
    _assert_grads_equal(ss, inp, device)


@pytest.mark.parametrize("size", [(736, 1424), (1040, 1008), (1040, 1040)], ids=["4094", "4095", "4225"])
def test_counts_around_the_packed_field(device, size):
    """The batched scan reads each rank's tile count from the 12 bits the depth sort's first pass
    packs above the Gaussian's 20-bit id, and looks a saturated count (>= 4095) up instead: grids of
    4094, 4095 and 4225 tiles, each with two splats that touch every tile among one-tile ones."""
    b = C.Builder(*size, seed=43)
    assert b.tiles == {(736, 1424): 4094, (1040, 1008): 4095, (1040, 1040): 4225}[size]
    for j in range(40):
        if j % 20 == 5:
            b.add_all_tiles(2.0 + 0.05 * j, 0.3)
        b.add_tile((97 * j + 3) % b.tiles, 2.0 + 0.05 * j + 0.01, opacity=0.4)
    cs = b.build("views_scan_packed", shuffle=True, n_absent=7)
    cams = [cs.cam] * 2 + gs_scenes.jittered_cameras(2, *size, seed=5, max_angle_deg=1.0, max_shift=0.02)[1:]
    ss = _settings(cams, 0, device)
    inp = _inputs(cs.scene, device)
    plain = _plain(ss, inp, 0)
    n0, _, _, e0 = plain[0]
    assert n0 == cs.I == 2 * b.tiles + 40 and int(e0["tiles_touched"].max()) == b.tiles
    assert np.array_equal(e0["point_list"].cpu().numpy(), cs.point_list)
    _assert_buffers_equal(plain, _buffers(ss, inp, 0, True))


def test_bounded_entry(device):
    """P = 1025, K = 3 bounded (binning_capacity above the counts, no count read back) equals the
    eager result; one capacity below its view's count raises through bounded_status()."""
    from diff_gaussian_rasterization import bounded_status

    ss = _settings(_cams(3), 1, device)
    inp = _inputs(_scene(1025, 1, seed=5 + 1025), device)
    plain = _plain(ss, inp, 1)
    counts = [n for n, _, _, _ in plain]
    cap = max(counts) + 1000
    _assert_buffers_equal(plain, _buffers(ss, inp, 1, True, capacity=cap))
    _assert_grads_equal(ss, inp, device, capacity=cap)
    assert bounded_status() == (0, 0)
    _preprocess(ss, inp, 1, capacity=[cap, counts[1] - 1, cap])
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="binning capacity"):
        bounded_status()
    assert bounded_status() == (0, 0)  # cleared


def test_above_the_look_back_limit(device):
    """P just past the last size of the look-back ordering (the tile counts travel with the depth
    sort's keys there): two views' scans batched over the carried counts."""
    cs = C.path_switch(C.LB_MAX_P + 1)
    cams = [cs.cam] + gs_scenes.jittered_cameras(2, cs.cam.image_width, cs.cam.image_height, seed=5,
                                                 max_angle_deg=1.0, max_shift=0.02)[1:]
    ss = _settings(cams, 0, device)
    inp = _inputs(cs.scene, device)
    plain = _plain(ss, inp, 0)
    assert plain[0][0] == cs.I
    _assert_buffers_equal(plain, _buffers(ss, inp, 0, True))


def _launches(fn):
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    torch.cuda.synchronize()
    lib.gs_profile_collect()
    lib.gs_profile_reset()
    lib.gs_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        return {k: n for k, (_, n) in _native.profile_stats().items()}
    finally:
        lib.gs_profile_enable(0)
        lib.gs_profile_reset()


def test_launch_names(device):
    """Two prepared views launch scan_reduce, scan_partials and scan_down once each and no scan_lb;
    a plain call and one prepared view still launch scan_lb."""
    ss = _settings(_cams(2), 1, device)
    inp = _inputs(_scene(1025, 1, seed=7), device)
    two = _launches(lambda: _preprocess(ss, inp, 1))
    assert [two.get(k, 0) for k in ("scan_reduce", "scan_partials", "scan_down", "scan_lb")] == [1, 1, 1, 0], two
    one = _launches(lambda: _preprocess(ss[:1], inp, 1))
    assert one.get("scan_lb", 0) == 1 and not any(k in one for k in ("scan_reduce", "scan_partials", "scan_down")), one
    plain = _launches(lambda: _buffers(ss[:1], inp, 1, False))
    assert plain.get("scan_lb", 0) == 1 and "scan_reduce" not in plain and "scan_down" not in plain, plain
