"""GPU tests of the K-view preprocess (prepare_views -> gs_forward_preprocess_views): the launch forms
each Gaussian's camera-independent half once (mean, 3D covariance, opacity, culling limit) and reads
its SH row once for all K cameras: held in registers (the default build), or -- a
-DGS_PREVIEWS_ROWS=1 build -- staged in LDS where the layout allows (whole 16-B rows of exactly
(D + 1)^2 coefficients at a 16-B aligned base: degrees 1 and 3) and by the per-lane loader
otherwise.  The cases cover both builds' paths; gs_debug_sh_rows_staged is the staged loader's
launch condition, checked here on the tensors' real addresses.  Every case compares the prepared path with K plain single-view calls, bit for bit:
images, radii, every field of _C.debug_export (splat-derived values of the visible rows, tile
counts, point list, ranges, final_T, n_contrib) and, after one backward per view, every gradient."""
import ctypes

import numpy as np
import pytest
import torch

import gs_scenes

pytestmark = pytest.mark.gpu

W, H = 70, 45  # neither a multiple of the 16-pixel tile


def _cams(K, w=W, h=H):
    return gs_scenes.jittered_cameras(K, w, h, seed=11, max_angle_deg=6.0, max_shift=0.3)


def _scene(P, deg, M=None, seed=3, cam=None):
    """A frustum-filling scene; M > (deg + 1)^2 pads the rows with coefficients the degree ignores."""
    cam = cam or gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(P, deg, cam=cam, seed=seed, scale_range=(0.02, 0.3))
    if M is not None and M != (deg + 1) ** 2:
        g = torch.Generator().manual_seed(seed + 100)
        pad = 0.05 * torch.randn((P, M - (deg + 1) ** 2, 3), generator=g)
        sc.shs = torch.cat([sc.shs, pad], 1).contiguous()
    return sc


def _staged(deg, shs):
    from diff_gaussian_rasterization import _native

    return _native.load().gs_debug_sh_rows_staged(deg, shs.shape[1], ctypes.c_void_p(shs.data_ptr()))


def _settings(cams, deg, device, scale_modifier=1.0):
    return [gs_scenes.raster_settings_for(c, deg, scale_modifier=scale_modifier, device=device) for c in cams]


def _buffers(ss, inp, deg, prepared, capacity=None):
    """Each view's (num_rendered, color, radii, debug_export dict) through _C, plain or prepared."""
    from diff_gaussian_rasterization import _C

    e = torch.Tensor([])
    g = lambda k: inp.get(k, e)  # noqa: E731
    s0 = ss[0]
    pre = [None] * len(ss)
    if prepared:
        pre = _C.preprocess_views([s.bg for s in ss], inp["means3D"], g("colors_precomp"), inp["opacities"],
                                  g("scales"), g("rotations"), s0.scale_modifier, g("cov3D_precomp"),
                                  [s.viewmatrix for s in ss], [s.projmatrix for s in ss], [s.tanfovx for s in ss],
                                  [s.tanfovy for s in ss], [s.image_height for s in ss], [s.image_width for s in ss],
                                  g("shs"), deg, [s.campos for s in ss], False, False, None,
                                  None if capacity is None else [capacity] * len(ss))
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


def _autograd(ss, inp, dpix, prepared, capacity=None, waits=None):
    """Each view's (image, radii, dL/dmeans2D) and the inputs' gradients summed over the views (one
    backward per view, in view order) through GaussianRasterizer, plain or with prepare_views."""
    from diff_gaussian_rasterization import GaussianRasterizer, _C, prepare_views

    leaves = {k: v.clone().requires_grad_(True) for k, v in inp.items()}
    rasts = [GaussianRasterizer(s) for s in ss]
    kw = {k: v for k, v in leaves.items() if k not in ("means3D", "opacities")}
    pre = [None] * len(ss)
    if prepared:
        with _C.row_waits(waits or []):
            pre = prepare_views(rasts, leaves["means3D"], leaves["opacities"], binning_capacity=capacity, **kw)
    outs = []
    for r, p, dp in zip(rasts, pre, dpix):
        m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
        img, radii = r(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], prepared=p, **kw)
        img.backward(dp)
        outs.append((img.detach().clone(), radii.clone(), m2.grad.clone()))
    torch.cuda.synchronize()
    return outs, {k: v.grad.clone() for k, v in leaves.items()}


def _assert_equal_paths(ss, inp, deg, device, capacity=None, waits=None):
    """The prepared path against K plain calls; returns the plain path's radii per view."""
    plain = _buffers(ss, inp, deg, False)
    prep = _buffers(ss, inp, deg, True)
    for v, ((na, ca, ra, ea), (nb, cb, rb, eb)) in enumerate(zip(plain, prep)):
        assert torch.equal(ca, cb) and torch.equal(ra, rb), v
        assert nb >= na  # views binned together share the largest count as their buffers' layout
        vis = ra > 0
        for k in ("xy", "conic_opacity", "rgb", "depth"):  # written for the visible rows only
            assert torch.equal(ea[k][vis], eb[k][vis]), (v, k)
        for k in ("tiles_touched", "ranges", "final_T", "n_contrib"):
            assert torch.equal(ea[k], eb[k]), (v, k)
        assert torch.equal(ea["point_list"], eb["point_list"][:na]), v
    dpix = [gs_scenes.dl_dimage(s.image_height, s.image_width, seed=40 + v, scale=1.0).to(device)
            for v, s in enumerate(ss)]
    a_out, a_grad = _autograd(ss, inp, dpix, False)
    b_out, b_grad = _autograd(ss, inp, dpix, True, capacity=capacity, waits=waits)
    for v, ((ia, ra, ma), (ib, rb, mb), (_, cp, rp, _)) in enumerate(zip(a_out, b_out, plain)):
        assert torch.equal(ia, ib) and torch.equal(ra, rb) and torch.equal(ma, mb), v
        assert torch.equal(ia, cp) and torch.equal(ra, rp), v
    for k in a_grad:
        assert torch.equal(a_grad[k], b_grad[k]), k
    return [ra for _, _, ra, _ in plain]


def _inputs(sc, device):
    d = sc.to(device)
    return dict(means3D=d.means3D, opacities=d.opacities, shs=d.shs, scales=d.scales, rotations=d.rotations)


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 2999])
def test_rows_and_degrees(device, P, deg):
    """Row counts around the 256-row workgroup (one lone row, the partial last workgroup) at every SH
    degree, M = (D + 1)^2: degrees 1 and 3 are eligible for the staged loader, 0 and 2 (3 M = 3, 27) are not."""
    inp = _inputs(_scene(P, deg), device)
    assert _staged(deg, inp["shs"]) == (1 if deg in (1, 3) else 0)
    radii = _assert_equal_paths(_settings(_cams(2), deg, device), inp, deg, device)
    assert P == 1 or all((r > 0).any() for r in radii)


@pytest.mark.parametrize("deg", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_view_counts(device, K, deg):
    """One view, a non-power of two and the launch's maximum of 8 views."""
    inp = _inputs(_scene(2999, deg, seed=5), device)
    radii = _assert_equal_paths(_settings(_cams(K), deg, device), inp, deg, device)
    assert all((r > 0).any() for r in radii)


def test_loader_fallback_layouts(device):
    """Layouts the staged loader must refuse, each still bit-identical to the plain calls: degree 1
    inside rows of M = 16, rows whose 3 M is not a multiple of 4 (M = 9, at degrees 1 and 2), and
    degree-3 rows at a base that is not 16-B aligned."""
    ss = lambda deg: _settings(_cams(3), deg, device)  # noqa: E731
    for deg, M in ((1, 16), (1, 9), (2, 9)):
        inp = _inputs(_scene(777, deg, M=M, seed=7), device)
        assert _staged(deg, inp["shs"]) == 0
        _assert_equal_paths(ss(deg), inp, deg, device)
    inp = _inputs(_scene(777, 3, seed=8), device)
    flat = torch.empty((inp["shs"].numel() + 1,), dtype=torch.float32, device=device)
    shs = flat[1:].view_as(inp["shs"])
    shs.copy_(inp["shs"])
    assert shs.data_ptr() % 16 == 4 and _staged(3, inp["shs"]) == 1 and _staged(3, shs) == 0
    inp["shs"] = shs
    _assert_equal_paths(ss(3), inp, 3, device)


def test_other_inputs(device):
    """colors_precomp, cov3D_precomp, and scale_modifier 0.7."""
    d = _scene(1500, 3, seed=9).to(device)
    gen = torch.Generator().manual_seed(2)
    colors = torch.rand((d.P, 3), generator=gen).to(device)
    base = dict(means3D=d.means3D, opacities=d.opacities)
    _assert_equal_paths(_settings(_cams(3), 0, device), dict(base, colors_precomp=colors, scales=d.scales,
                                                              rotations=d.rotations), 0, device)
    s2 = (d.scales ** 2)
    zero = torch.zeros_like(s2[:, 0])
    cov = torch.stack([s2[:, 0], 0.3 * s2[:, 0], zero, s2[:, 1] + s2[:, 0], zero, s2[:, 2]], 1).contiguous()
    _assert_equal_paths(_settings(_cams(3), 3, device), dict(base, shs=d.shs, cov3D_precomp=cov), 3, device)
    _assert_equal_paths(_settings(_cams(3), 3, device, scale_modifier=0.7),
                        dict(base, shs=d.shs, scales=d.scales, rotations=d.rotations), 3, device)


def test_one_tile_image(device):
    """A 16 x 16 image: one tile."""
    cams = _cams(2, 16, 16)
    inp = _inputs(_scene(600, 3, seed=12, cam=cams[0]), device)
    _assert_equal_paths(_settings(cams, 3, device), inp, 3, device)


def test_culling_that_differs_between_views(device):
    """Three cameras and three constructed groups of Gaussians (covariances given as cov3D_precomp):
      A  behind camera 0's near plane (z <= 0.2), in front of camera 1, which looks back from z = 2 fx;
      B  on the axis: visible to cameras 0 and 1, far outside the frame of camera 2 (camera 0 moved
         40 units sideways), which A is also behind;
      C  zero determinant in every view: cov3D = diag(-0.3, 0, 0) at depth fx from each camera, where
         the EWA Jacobian's fx / z is exactly 1, so cov2D = (-0.3 + 0.3, 0, 0.3) and det == 0;
    then random filler.  A row culled by one camera must not suppress its later views, and what the
    launch shares between the views must not depend on the first one."""
    s0 = _settings([gs_scenes.identity_camera(W, H)], 3, device)[0]
    fx = float(np.float32(W) / (np.float32(2.0) * np.float32(s0.tanfovx)))  # the library's fx, in float32
    cams = [gs_scenes.identity_camera(W, H),
            gs_scenes.look_at_camera((0.0, 0.0, 2.0 * fx), (0.0, 0.0, 0.0), W, H),
            gs_scenes.make_camera(np.eye(3), np.array([-40.0, 0.0, 0.0]), W, H)]
    g = torch.Generator().manual_seed(17)
    nA, nB, nC, nF = 40, 40, 20, 200
    xy = lambda n, r: (2 * torch.rand((n, 2), generator=g) - 1) * r  # noqa: E731
    A = torch.cat([xy(nA, 0.5), -3.0 - torch.rand((nA, 1), generator=g)], 1)
    B = torch.cat([xy(nB, 0.3), 3.0 + 3.0 * torch.rand((nB, 1), generator=g)], 1)
    C = torch.cat([xy(nC, 2.0), torch.full((nC, 1), fx)], 1)
    fill = _scene(nF, 3, seed=18)
    means = torch.cat([A, B, C, fill.means3D], 0).contiguous()
    P = means.shape[0]
    s2 = 0.01 + 0.05 * torch.rand((P, 3), generator=g)
    zero = torch.zeros((P,))
    cov = torch.stack([s2[:, 0], zero, zero, s2[:, 1], zero, s2[:, 2]], 1)
    cov[nA + nB:nA + nB + nC] = torch.tensor([-0.3, 0.0, 0.0, 0.0, 0.0, 0.0])
    sc = _scene(P, 3, seed=19)
    inp = dict(means3D=means.to(device), opacities=sc.opacities.to(device), shs=sc.shs.to(device),
               cov3D_precomp=cov.contiguous().to(device))
    radii = _assert_equal_paths(_settings(cams, 3, device), inp, 3, device)
    iA, iB, iC = slice(0, nA), slice(nA, nA + nB), slice(nA + nB, nA + nB + nC)
    want = [(False, True, False), (True, True, False), (False, False, False)]  # visible: (A, B, C) per view
    for v, (r, w) in enumerate(zip(radii, want)):
        for name, idx, vis in zip("ABC", (iA, iB, iC), w):
            assert bool((r[idx] > 0).all()) if vis else bool((r[idx] == 0).all()), (v, name)


def test_bounded_entry(device):
    """The same comparison with the prepared views bounded (binning_capacity=, no count read back)."""
    for deg in (1, 3):
        inp = _inputs(_scene(2999, deg, seed=21), device)
        _assert_equal_paths(_settings(_cams(3), deg, device), inp, deg, device, capacity=200_000)


def test_row_waits_inside_a_workgroup(device):
    """Row waits installed (events already complete), two chunks whose boundary lies inside a
    workgroup: the chunked launch equals the unchunked one and the plain calls."""
    inp = _inputs(_scene(2999, 3, seed=23), device)
    ev = torch.cuda.Event()
    ev.record()
    torch.cuda.synchronize()
    _assert_equal_paths(_settings(_cams(3), 3, device), inp, 3, device, waits=[(0, 300, ev), (300, 2999, ev)])


# ------------------------------------------------------------------------------------------
# views of different sizes
# ------------------------------------------------------------------------------------------
# The bridges (_C.preprocess_views and its twin in gs_torch_ext.cpp) batch the K views' binning only
# when every view has one W x H; otherwise each view bins itself inside its own prepared render,
# behind the shared preprocess (k_preprocess_views with per-view gx, gy) and ordering.
# Every comparison below is bit for bit (torch.equal): there is no bound, the gradient-to-bound
# ratio of these tests is 0 by assertion (MI355X: all equal).
MIXED_SIZES = {
    # 256 tiles = 8 tile bits (one tile-sort pass), 272 tiles = 9 bits (two passes), and a ragged 5 x 3 grid
    "three_sort_plans": [(256, 256), (272, 256), (70, 45)],
    "one_tile_and_many": [(16, 16), (203, 117)],
    "portrait_landscape": [(117, 203), (203, 117)],
    # only the last of the launch's maximum of 8 views differs
    "last_of_eight": [(70, 45)] * 7 + [(45, 70)],
}


def _mixed_cams(sizes):
    """View k has the k-th pose of _cams at its own image size (the poses do not depend on the size)."""
    return [_cams(k + 1, w, h)[k] for k, (w, h) in enumerate(sizes)]


def _mixed_scene(sizes, P, deg, seed):
    """Fills the frustum of the narrowest half-angles among the views, so every view sees it."""
    w, h = min(sizes, key=lambda s: s[0] / s[1])  # the narrowest horizontal field (fovy is fixed)
    return _scene(P, deg, seed=seed, cam=gs_scenes.identity_camera(w, h))


@pytest.fixture(params=["ext", "ctypes"])
def bridge(request, monkeypatch):
    """Both implementations of preprocess_views / the prepared render: the torch C++ binding (the
    default path) and the ctypes one (_C._EXT patched away, as tests/test_gpu_ext.py does)."""
    from diff_gaussian_rasterization import _C

    if request.param == "ext":
        assert _C._EXT is not None, "the torch C++ host path (_gs_ext) is not loaded"
    else:
        monkeypatch.setattr(_C, "_EXT", None)
    return request.param


@pytest.mark.parametrize("deg", [1, 3])
@pytest.mark.parametrize("name", list(MIXED_SIZES))
def test_views_of_different_sizes(device, bridge, name, deg):
    """Unequal image sizes in one prepare_views call, through both bridges: every view bit-equal to
    its plain single-view call (images, radii, every debug_export field, every gradient)."""
    sizes = MIXED_SIZES[name]
    assert len(set(sizes)) > 1
    inp = _inputs(_mixed_scene(sizes, 2999, deg, seed=31), device)
    radii = _assert_equal_paths(_settings(_mixed_cams(sizes), deg, device), inp, deg, device)
    assert all((r > 0).any() for r in radii)


def test_views_of_different_sizes_precomputed_colors(device, bridge):
    """colors_precomp (no SH rows to share) with three sizes."""
    sizes = MIXED_SIZES["three_sort_plans"]
    d = _mixed_scene(sizes, 1500, 0, seed=33).to(device)
    colors = torch.rand((d.P, 3), generator=torch.Generator().manual_seed(4)).to(device)
    inp = dict(means3D=d.means3D, opacities=d.opacities, colors_precomp=colors, scales=d.scales, rotations=d.rotations)
    radii = _assert_equal_paths(_settings(_mixed_cams(sizes), 0, device), inp, 0, device)
    assert all((r > 0).any() for r in radii)


def test_views_of_different_sizes_bounded(device, bridge):
    """Unequal sizes with the prepared views bounded (binning_capacity=): each view sizes its own
    binning buffer for the capacity and its own grid."""
    sizes = MIXED_SIZES["three_sort_plans"]
    inp = _inputs(_mixed_scene(sizes, 2999, 3, seed=35), device)
    radii = _assert_equal_paths(_settings(_mixed_cams(sizes), 3, device), inp, 3, device, capacity=200_000)
    assert all((r > 0).any() for r in radii)


def test_views_of_different_sizes_row_waits(device):
    """Unequal sizes with row waits installed, the chunk boundary inside a workgroup."""
    sizes = MIXED_SIZES["portrait_landscape"]
    inp = _inputs(_mixed_scene(sizes, 2999, 3, seed=37), device)
    ev = torch.cuda.Event()
    ev.record()
    torch.cuda.synchronize()
    radii = _assert_equal_paths(_settings(_mixed_cams(sizes), 3, device), inp, 3, device,
                                waits=[(0, 300, ev), (300, 2999, ev)])
    assert all((r > 0).any() for r in radii)


@pytest.mark.parametrize("deg", [1, 3])
def test_unbatched_fallback_equals_batched_binning(device, monkeypatch, deg):
    """The same-size control: three views of one size through the ctypes bridge, binned together (the
    default) and -- GSRAST_BATCH_VIEWS=0, which that bridge reads at every call -- each inside its
    own prepared render, the path views of unequal sizes take.  Bit for bit the same buffers and
    gradients, and both equal to the plain calls."""
    from diff_gaussian_rasterization import _C

    monkeypatch.setattr(_C, "_EXT", None)
    ss = _settings(_cams(3), deg, device)
    inp = _inputs(_scene(2999, deg, seed=39), device)
    dpix = [gs_scenes.dl_dimage(H, W, seed=60 + v, scale=1.0).to(device) for v in range(3)]
    monkeypatch.delenv("GSRAST_BATCH_VIEWS", raising=False)
    batched = _buffers(ss, inp, deg, True)
    b_out, b_grad = _autograd(ss, inp, dpix, True)
    monkeypatch.setenv("GSRAST_BATCH_VIEWS", "0")
    single = _buffers(ss, inp, deg, True)
    s_out, s_grad = _autograd(ss, inp, dpix, True)
    radii = _assert_equal_paths(ss, inp, deg, device)  # the fallback against the plain calls
    assert all((r > 0).any() for r in radii)
    counts = [n for n, _, _, _ in single]
    assert len(set(counts)) > 1                              # each view kept its own count: not batched
    assert all(n == max(counts) for n, _, _, _ in batched)  # binned together: the largest count for all
    for v, ((nb, cb, rb, eb), (ns, cs, rs, es)) in enumerate(zip(batched, single)):
        assert torch.equal(cb, cs) and torch.equal(rb, rs), v
        vis = rs > 0
        for k in ("xy", "conic_opacity", "rgb", "depth"):
            assert torch.equal(eb[k][vis], es[k][vis]), (v, k)
        for k in ("tiles_touched", "ranges", "final_T", "n_contrib"):
            assert torch.equal(eb[k], es[k]), (v, k)
        assert torch.equal(eb["point_list"][:ns], es["point_list"]), v
    for v, (b, s) in enumerate(zip(b_out, s_out)):
        assert all(torch.equal(x, y) for x, y in zip(b, s)), v
    for k in b_grad:
        assert torch.equal(b_grad[k], s_grad[k]), k
