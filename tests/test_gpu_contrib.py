"""Per-Gaussian contribution statistics (gs_importance.view_contributions, gs_contrib_stats) and the
pruning built on them, on the GPU.

The scenes are tests/test_gpu_aux.py's, built the same way through gs_scenes.identity_camera(200, 120)
(not a multiple of the 16-px tile either way, so edge tiles have lanes outside the image):

    sparse      random_gaussians(2000, 3, seed=41): one staged batch per tile
    deep        random_gaussians(6000, 1, seed=47, scale_range=(0.01, 0.08)): two or three batches
    opaque      random_gaussians(8000, 1, seed=49, scale_range=(0.02, 0.12)), opacities 0.5 + 0.49 o:
                T-stopped pixels, up to five batches
    empty-tile  the first 3 Gaussians of `sparse` at 72 x 40: tiles with n_eff == 0
    sparse-low  `sparse` with a seeded third of the opacities (torch.rand(2000, manual_seed(7)) < 1/3)
                set to 0.003 < 1/255: never composited

Every check runs in both numerics modes (gs_set_exact_exp), with and without a weight map, with and
without accumulation, so both walk instantiations and the reduce are launched in this process
(tests/test_zz_kernel_coverage.py).

1. Bit identities: run to run; no map == a map of ones; forward -> stats -> backward leaves the
   backward's gradients, the colour, final_T and n_contrib bit-identical to forward -> backward (and
   stats after the backward equal stats before it); two views accumulated with out= equal the
   separate results combined in torch; radii == 0 => (0, 0, 0); count == 0 <=> wmax == 0 <=> wsum == 0;
   0 <= wmax <= 0.99; count <= the pixel area of the tile rectangle; P == 0 and a zero map give zeros.
2. Telescoping: sum_i wsum[i] (fp64) against sum_p alpha_p of an aux render, within
   sum_p 2 n_contrib[p] 2^-24 (two roundings per composited entry of the telescoping product, the
   derivation of tests/test_gpu_aux.py section 2) + 2^-16 sum_i wsum[i] (a tile entry's at most 256
   positive terms summed in fp32 in any order).
3. Against the existing path: wsum under a random positive map m against dL/dcolors_precomp[:, 0]
   of a plain call with dL/dimage = (m, 0, 0), within twice test_gpu_dense._check's bound.
4. Against the fp64 dense reference (dense_ref_contrib.contributions_local, flag_rel=1e-3,
   flag_T_rel=1e-2; m zeroed at flagged pixels and in the widened rectangles of Gaussians whose
   radius differs): count exactly; wsum and wmax by the conditioning rule of test_gpu_dense,
   max|hip - f64| <= 4 max|dense f32 - f64| + 1e-5 max|ref|.
5. Pruning keeps the image: on sparse-low count > 0 drops exactly the lowered third and the render
   of the pruned inputs equals the full render bit for bit; the same through gs_importance.prune on
   a model with a FusedAdam.
6. Interface: antialiasing=True against the plain call given the compensated opacities; the refused
   inputs and maps.
"""
import math

import numpy as np
import pytest
import torch

import dense_cases
import dense_ref_aa
import dense_ref_contrib
import gs_scenes
from gpu_checks import check_4x, check_tol, mode  # noqa: F401

pytestmark = pytest.mark.gpu

def _map(cam, device, seed=13):
    """a random positive weight map in [0.25, 1.25)"""
    g = torch.Generator().manual_seed(seed)
    return (0.25 + torch.rand((cam.image_height, cam.image_width), generator=g)).to(device)


def _rasterizer(cam, deg, device):
    from diff_gaussian_rasterization import GaussianRasterizer

    return GaussianRasterizer(gs_scenes.raster_settings_for(cam, deg, device=device))


def _inputs(leaves, **over):
    kw = dict(means3D=leaves["means3D"], opacities=leaves["opacities"], shs=leaves["shs"], scales=leaves["scales"],
              rotations=leaves["rotations"])
    kw.update(over)
    return kw


def _stats(cam, leaves, deg, device, **kw):
    import gs_importance

    st = gs_importance.view_contributions(_rasterizer(cam, deg, device), **kw, **_inputs(leaves))
    torch.cuda.synchronize()
    return st


def _render(cam, leaves, deg, device, aux=False, **over):
    with torch.no_grad():
        kw = _inputs(leaves, **over)
        out = _rasterizer(cam, deg, device)(means2D=torch.zeros_like(kw["means3D"]), aux_outputs=aux, **kw)
    torch.cuda.synchronize()
    return out


def _raw(cam, leaves, deg, device, dpix, stats):
    """forward -> (stats) -> backward -> (stats) through the raw _C calls"""
    from diff_gaussian_rasterization import _C

    s = gs_scenes.raster_settings_for(cam, deg, device=device)
    e = torch.Tensor([])
    H, W = s.image_height, s.image_width
    with torch.no_grad():
        R, color, radii, geom, binning, img = _C.rasterize_gaussians_two_call(
            s.bg, leaves["means3D"], e, leaves["opacities"], leaves["scales"], leaves["rotations"], s.scale_modifier,
            e, s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, H, W, leaves["shs"], s.sh_degree, s.campos,
            s.prefiltered, s.debug)

        def cs():
            return _C.contribution_stats(R, radii, geom, binning, img, s.viewmatrix, s.projmatrix, s.campos,
                                         s.tanfovx, s.tanfovy, H, W)

        before = cs() if stats else None
        grads = _C.rasterize_gaussians_backward(
            s.bg, leaves["means3D"], radii, e, leaves["scales"], leaves["rotations"], s.scale_modifier, e,
            s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, dpix, leaves["shs"], s.sh_degree, s.campos, geom, R,
            binning, img, s.debug)
        after = cs() if stats else None
        ex = _C.debug_export(leaves["means3D"].shape[0], W, H, R, geom, binning, img, device)
    torch.cuda.synchronize()
    return color, radii, grads, ex, before, after


# ------------------------------------------------------------------------------------------
# 1. bit identities
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "opaque", "empty-tile"])
def test_bit_identities(device, mode, name):
    import gs_importance

    cam, leaves, deg = dense_cases.scene(name, device)
    H, W = cam.image_height, cam.image_width
    P = leaves["means3D"].shape[0]
    m = _map(cam, device)
    a, b = _stats(cam, leaves, deg, device), _stats(cam, leaves, deg, device)
    am, bm = _stats(cam, leaves, deg, device, pixel_weights=m), _stats(cam, leaves, deg, device, pixel_weights=m[None])
    for x, y in ((a, b), (am, bm)):  # (a) run to run
        for f, u, v in zip(x._fields, x, y):
            assert torch.equal(u, v), f"{f} differs run to run"
    assert a.wsum.dtype == a.wmax.dtype == torch.float32 and a.count.dtype == a.radii.dtype == torch.int32
    assert a.wsum.shape == a.wmax.shape == a.count.shape == a.radii.shape == (P,)
    one = _stats(cam, leaves, deg, device, pixel_weights=torch.ones((H, W), device=device))
    for f, u, v in zip(a._fields, a, one):  # (b)
        assert torch.equal(u, v), f"{f}: no map differs from a map of ones"
    assert not torch.equal(a.wsum, am.wsum) and torch.equal(a.count, am.count)

    # (c) the statistics leave the view's backward alone, and it them
    dpix = gs_scenes.dl_dimage(H, W, seed=5, scale=1.0).to(device)
    c0, r0, g0, ex0, _, _ = _raw(cam, leaves, deg, device, dpix, stats=False)
    c1, r1, g1, ex1, before, after = _raw(cam, leaves, deg, device, dpix, stats=True)
    assert torch.equal(c0, c1) and torch.equal(r0, r1)
    for k in ("final_T", "n_contrib", "point_list", "ranges"):
        assert torch.equal(ex0[k], ex1[k]), k
    assert len(g0) == len(g1) == 8
    for k, (u, v) in enumerate(zip(g0, g1)):
        assert torch.equal(u, v), f"gradient {k} differs after the statistics"
    for f, u, v, w in zip(a._fields, before, after, a):
        assert torch.equal(u, v), f"{f}: after the backward differs from before it"
        assert torch.equal(u, w), f"{f}: the raw call differs from view_contributions"
    assert torch.equal(r0, a.radii)

    # (d) two views accumulated in place
    cam2 = gs_scenes.jittered_cameras(2, W, H)[1]
    m2 = _map(cam, device, seed=14)
    for maps in ((None, None), (m, m2)):
        va = _stats(cam, leaves, deg, device, pixel_weights=maps[0])
        vb = _stats(cam2, leaves, deg, device, pixel_weights=maps[1])
        acc = _stats(cam, leaves, deg, device, pixel_weights=maps[0])
        ret = _stats(cam2, leaves, deg, device, pixel_weights=maps[1], out=acc)
        assert ret.wsum.data_ptr() == acc.wsum.data_ptr() and ret.count.data_ptr() == acc.count.data_ptr()
        assert torch.equal(ret.wsum, va.wsum + vb.wsum)
        assert torch.equal(ret.wmax, torch.maximum(va.wmax, vb.wmax))
        assert torch.equal(ret.count, va.count + vb.count)
        assert torch.equal(ret.radii, vb.radii)
        both = gs_importance.accumulate_views([_rasterizer(cam, deg, device), _rasterizer(cam2, deg, device)],
                                              pixel_weights=None if maps[0] is None else list(maps), **_inputs(leaves))
        for f, u, v in zip(ret._fields, ret, both):
            assert torch.equal(u, v), f"accumulate_views: {f}"
    assert not torch.equal(va.wsum, vb.wsum)

    for st in (a, am):
        zero = st.radii == 0
        for t in st[:3]:  # (e)
            assert not t[zero].any()
        # (f) with a positive map
        assert torch.equal(st.count == 0, st.wmax == 0) and torch.equal(st.count == 0, st.wsum == 0)
        assert bool((st.count >= 0).all()) and bool((st.wsum >= st.wmax).all())
    assert float(a.wmax.min()) >= 0.0 and float(a.wmax.max()) <= 0.99  # (g)
    assert float(a.wmax.max()) > 0.0 and int(a.count.max()) > 0
    if name != "empty-tile":
        assert float(a.wmax.max()) > 0.3 and int(a.count.max()) > 10
    # (h) at most the pixels of the tile rectangle
    assert bool((a.count.long() <= 256 * ex0["tiles_touched"].long()).all())
    if name == "empty-tile":
        assert int((ex0["ranges"][:, 1] == ex0["ranges"][:, 0]).sum()) >= 1

    # (i) a zero map, and no Gaussians
    z = _stats(cam, leaves, deg, device, pixel_weights=torch.zeros((H, W), device=device))
    for t in z[:3]:
        assert not t.any()
    assert torch.equal(z.radii, a.radii)
    none = _stats(cam, {k: v[:0].contiguous() for k, v in leaves.items()}, deg, device)
    for t in none:
        assert t.shape == (0,)


# ------------------------------------------------------------------------------------------
# 2. telescoping
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "deep", "opaque", "empty-tile"])
def test_wsum_telescopes_to_alpha(device, mode, name):
    cam, leaves, deg = dense_cases.scene(name, device)
    H, W = cam.image_height, cam.image_width
    st = _stats(cam, leaves, deg, device)
    _, _, _, alpha = _render(cam, leaves, deg, device, aux=True)
    dpix = torch.zeros((3, H, W), device=device)
    ex = _raw(cam, leaves, deg, device, dpix, stats=False)[3]
    total, want = float(st.wsum.double().sum()), float(alpha.double().sum())
    bound = 2.0 * float(ex["n_contrib"].double().sum()) * 2.0 ** -24 + 2.0 ** -16 * total
    print(f"\n[{name}] sum wsum {total:.9e}  sum alpha {want:.9e}  |d| {abs(total - want):.3e}  bound {bound:.3e} "
          f"({abs(total - want) / bound:.3f} of it)")
    assert want > 0 and abs(total - want) <= bound
    # every composited (pixel, entry) pair is one hit: at most n_contrib entries per pixel
    assert int(st.count.long().sum()) <= int(ex["n_contrib"].long().sum())


# ------------------------------------------------------------------------------------------
# 3. against the existing path
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "deep", "opaque"])
def test_wsum_against_the_colour_gradient(device, mode, name):
    cam, leaves, deg = dense_cases.scene(name, device)
    H, W = cam.image_height, cam.image_width
    P = leaves["means3D"].shape[0]
    m = _map(cam, device)
    st = _stats(cam, leaves, deg, device, pixel_weights=m)
    cols = torch.rand((P, 3), generator=torch.Generator().manual_seed(3)).to(device).requires_grad_(True)
    kw = _inputs(leaves, shs=None, colors_precomp=cols)
    img, radii = _rasterizer(cam, deg, device)(means2D=torch.zeros_like(leaves["means3D"]), **kw)
    (img[0] * m).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(radii, st.radii)
    print()
    check_tol(st.wsum, cols.grad[:, 0], f"[{name}] wsum vs dL/dcolors_precomp[:, 0]", times=2)


# ------------------------------------------------------------------------------------------
# 4. against the fp64 dense reference
# ------------------------------------------------------------------------------------------
_DENSE = {}


def _dense(name, cam, leaves, deg, device, dtype, weights, **flags):
    t = {k: v.detach().to(dtype) for k, v in leaves.items()}
    return dense_ref_contrib.contributions_local(
        t["means3D"], t["means2D"], t["opacities"], *dense_cases.dense_args(cam, device, dtype), weights=weights,
        shs=t["shs"], deg=deg, scales=t["scales"],
        rots=t["rotations"], **flags)


def _dense_case(name, cam, leaves, deg, device, hip_radii):
    """The weight map (zero at the flagged pixels) and the fp64 / fp32 dense statistics under it; the
    dense side does not depend on the kernels' numerics mode: computed once per scene and set of
    differing radii."""
    c = _DENSE.setdefault(name, {})
    if "rect" not in c:
        c["rect"], c["radii"] = dense_cases.rect_and_radii(cam, leaves, deg, device)
    rdiff = (hip_radii.cpu() != c["radii"]).numpy()
    wide = dense_cases.wide_mask(c["rect"], rdiff, cam.image_width, cam.image_height)
    if "wide" not in c or not np.array_equal(c["wide"], wide):
        c["wide"] = wide
        c["f64"] = _dense(name, cam, leaves, deg, device, torch.float64, _map(cam, device, seed=17).double(),
                          flag_rel=1e-3, flag_T_rel=1e-2, zero_flagged=True, also_flag=torch.from_numpy(wide))
        c["m"] = c["f64"]["weights"].float()
        c["f32"] = _dense(name, cam, leaves, deg, device, torch.float32, c["m"])
    fl = c["f64"]["flag"].cpu().numpy() | wide
    assert torch.equal(c["m"] == 0, torch.from_numpy(fl).to(device))
    return c["m"], fl, rdiff, c["f64"], c["f32"]


@pytest.mark.parametrize("name", ["sparse", "deep", "opaque"])
def test_against_dense_fp64(device, mode, name):
    cam, leaves, deg = dense_cases.scene(name, device)
    P = leaves["means3D"].shape[0]
    radii = _stats(cam, leaves, deg, device).radii
    m, fl, rdiff, r64, r32 = _dense_case(name, cam, leaves, deg, device, radii)
    print(f"\n[{name}] flagged pixels {int(fl.sum())}/{fl.size} ({fl.mean():.4f}), radii differing "
          f"{int(rdiff.sum())}/{P}")
    assert fl.mean() <= 0.02
    assert rdiff.mean() <= 1e-3, f"{int(rdiff.sum())} radii differ"
    st = _stats(cam, leaves, deg, device, pixel_weights=m)
    keep = ~rdiff
    cnt, ref_cnt = st.count.long().cpu().numpy()[keep], r64["count"].cpu().numpy()[keep]
    c32 = r32["count"].cpu().numpy()[keep]
    print(f"  count: {int((cnt != ref_cnt).sum())} of {cnt.size} differ from f64 (dense f32: "
          f"{int((c32 != ref_cnt).sum())}), max {int(ref_cnt.max())}")
    assert int(ref_cnt.max()) > 10
    assert np.array_equal(cnt, ref_cnt)
    check_4x(st.wsum, r64["wsum"], r32["wsum"], f"[{name}] wsum", keep)
    check_4x(st.wmax, r64["wmax"], r32["wmax"], f"[{name}] wmax", keep)


# ------------------------------------------------------------------------------------------
# 5. pruning keeps the image
# ------------------------------------------------------------------------------------------
def test_pruning_keeps_the_image(device, mode):
    cam, leaves, deg = dense_cases.scene("sparse-low", device)
    low = dense_cases.lowered().to(device)
    assert 600 < int(low.sum()) < 740
    img, radii, _, alpha = _render(cam, leaves, deg, device, aux=True)
    # a pixel can only have stopped if its T fell below 0.01: removing a never-composited Gaussian is
    # exactly neutral where no pixel stopped on it
    assert float(alpha.max()) <= 0.98
    st = _stats(cam, leaves, deg, device)
    keep = st.count > 0
    assert torch.equal(~keep, low), f"{int((~keep & ~low).sum())} others never composited, " \
                                    f"{int((keep & low).sum())} lowered ones composited"
    pruned = {k: v[keep].contiguous() for k, v in leaves.items()}
    img_p, radii_p = _render(cam, pruned, deg, device)
    assert torch.equal(img_p, img) and torch.equal(radii_p, radii[keep])


def test_prune_on_a_model_with_fused_adam(device, mode):
    import gs_importance
    import gs_train

    cam, leaves, deg = dense_cases.scene("sparse-low", device)
    P = leaves["means3D"].shape[0]

    class Model:
        pass

    g = torch.Generator().manual_seed(23)
    mdl = Model()
    op = leaves["opacities"]
    raw = dict(_xyz=leaves["means3D"], _features_dc=leaves["shs"][:, :1], _features_rest=leaves["shs"][:, 1:],
               _opacity=torch.log(op / (1 - op)), _scaling=torch.log(leaves["scales"]), _rotation=leaves["rotations"])
    names = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
    groups = []
    for n, (a, v) in zip(names, raw.items()):
        p = torch.nn.Parameter(v.detach().clone().contiguous())
        setattr(mdl, a, p)
        groups.append({"params": [p], "lr": 0.0, "name": n})
    mdl.optimizer = gs_train.FusedAdam(groups, lr=0.0, eps=1e-15)
    for grp in groups:
        p = grp["params"][0]
        p.grad = torch.randn(p.shape, generator=g).to(device)
    mdl.optimizer.step()
    mdl.xyz_gradient_accum = torch.rand((P, 1), generator=g).to(device)
    mdl.denom = torch.rand((P, 1), generator=g).to(device)
    mdl.max_radii2D = torch.rand((P,), generator=g).to(device)

    def model_leaves():
        with torch.no_grad():
            x, shs, o, s, q = gs_train.render_inputs(mdl)
        return dict(means3D=x.detach(), opacities=o, shs=shs, scales=s, rotations=q)

    full = model_leaves()
    assert float((full["opacities"] - op).abs().max()) <= 1e-6  # (the activations round-trip to an ulp)
    img, radii, _, alpha = _render(cam, full, deg, device, aux=True)
    assert float(alpha.max()) <= 0.98
    st = _stats(cam, full, deg, device)
    keep = gs_importance.keep_mask(st, min_count=1)
    assert torch.equal(~keep, dense_cases.lowered().to(device))
    old = {a: getattr(mdl, a) for a in raw}
    want = {a: old[a].detach()[keep].clone() for a in raw}
    mom = {a: {k: (v if k == "step" else v[keep].clone()) for k, v in mdl.optimizer.state[old[a]].items()}
           for a in raw}
    stats = [getattr(mdl, n)[keep].clone() for n in ("xyz_gradient_accum", "denom", "max_radii2D")]
    gs_importance.prune(mdl, keep)
    by_name = {grp["name"]: grp for grp in mdl.optimizer.param_groups}
    for n, a in zip(names, raw):
        p = getattr(mdl, a)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and by_name[n]["params"][0] is p
        assert torch.equal(p.detach(), want[a]) and old[a] not in mdl.optimizer.state
        s2 = mdl.optimizer.state[p]
        assert torch.equal(s2["exp_avg"], mom[a]["exp_avg"]) and torch.equal(s2["exp_avg_sq"], mom[a]["exp_avg_sq"])
        assert float(s2["step"]) == float(mom[a]["step"]) == 1.0
    for got, ref in zip((mdl.xyz_gradient_accum, mdl.denom, mdl.max_radii2D), stats):
        assert torch.equal(got, ref)
    img_p, radii_p = _render(cam, model_leaves(), deg, device)
    assert torch.equal(img_p, img) and torch.equal(radii_p, radii[keep])
    # and the optimizer steps the pruned model
    for grp in mdl.optimizer.param_groups:
        grp["params"][0].grad = torch.zeros_like(grp["params"][0])
    mdl.optimizer.step()
    torch.cuda.synchronize()
    assert float(mdl.optimizer.state[mdl._xyz]["step"]) == 2.0


# ------------------------------------------------------------------------------------------
# 6. interface
# ------------------------------------------------------------------------------------------
def test_antialiasing_equals_the_plain_call_with_the_compensated_opacities(device, mode):
    cam, leaves, deg = dense_cases.scene("sparse", device)
    H, W = cam.image_height, cam.image_width
    m = _map(cam, device)
    s = dense_ref_aa.aa_scale(leaves["means3D"], cam.world_view_transform.to(device), math.tan(cam.FoVx / 2),
                              math.tan(cam.FoVy / 2), W, H, scales=leaves["scales"], rots=leaves["rotations"])
    eff = (leaves["opacities"] * s[:, None]).contiguous()
    assert float(s.min()) < 0.9 and float(s.max()) < 1.0
    aa = _stats(cam, leaves, deg, device, pixel_weights=m, antialiasing=True)
    plain = _stats(cam, dict(leaves, opacities=eff), deg, device, pixel_weights=m)
    off = _stats(cam, leaves, deg, device, pixel_weights=m)
    assert torch.equal(aa.radii, plain.radii) and not torch.equal(aa.wsum, off.wsum)
    print()
    check_tol(aa.wsum, plain.wsum, "antialiased wsum vs compensated opacities", times=2)
    check_tol(aa.wmax, plain.wmax, "antialiased wmax vs compensated opacities", times=2)
    check_tol(aa.count, plain.count, "antialiased count vs compensated opacities", times=2)


def test_refused_inputs(device):
    import gs_importance

    cam, leaves, deg = dense_cases.scene("sparse", device)
    H, W = cam.image_height, cam.image_width
    r = _rasterizer(cam, deg, device)
    kw = _inputs(leaves)
    with pytest.raises(Exception, match="Please provide excatly one of either SHs or precomputed colors!"):
        gs_importance.view_contributions(r, **dict(kw, shs=None))
    with pytest.raises(Exception, match="Please provide excatly one of either SHs or precomputed colors!"):
        gs_importance.view_contributions(r, **dict(kw, colors_precomp=leaves["means3D"]))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        gs_importance.view_contributions(r, **dict(kw, scales=None))
    with pytest.raises(RuntimeError, match="needs device tensors; means3D is on cpu"):
        gs_importance.view_contributions(r, **dict(kw, means3D=leaves["means3D"].cpu()))
    with pytest.raises(RuntimeError, match="opacities"):
        gs_importance.view_contributions(r, **dict(kw, opacities=leaves["opacities"].cpu()))
    for bad in (torch.ones((H, W + 1), device=device), torch.ones((3, H, W), device=device), torch.ones((H, W)),
                torch.ones((H, W), device=device, dtype=torch.float64), torch.ones((W, H), device=device)):
        with pytest.raises(ValueError, match="pixel_weights"):
            gs_importance.view_contributions(r, pixel_weights=bad, **kw)
    st = gs_importance.view_contributions(r, **kw)
    with pytest.raises(ValueError, match="out.count"):
        gs_importance.view_contributions(r, out=st._replace(count=st.count.float()), **kw)
    with pytest.raises(ValueError, match="out.wsum"):
        gs_importance.view_contributions(r, out=st._replace(wsum=st.wsum[:-1]), **kw)
    with pytest.raises(ValueError, match="one pixel_weights entry per view"):
        gs_importance.accumulate_views([r, r], pixel_weights=[None], **kw)
    torch.cuda.synchronize()
