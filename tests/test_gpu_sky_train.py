"""train_step with the skysphere and a depth prior (gs_train_step.train_step(sky=, depth_prior=)):
the fused backward + Adam step (fuse_adam=True) takes the alpha / inverse-depth gradients through
the deferred aux backward (gs_backward_render_aux, gs_backward_gaussians_adam_stats_aux) and must
equal the unfused step bit for bit.  Shapes are test_train_step.py's: 3000 / 2999 Gaussians,
160 x 120 (80 tiles), a 16 x 32 sky texture, bg zero."""
import os

import numpy as np
import pytest
import torch

import gs_scenes

pytestmark = pytest.mark.gpu

NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
W, H = 160, 120
PARAMS = [(3, 3000), (2, 3000), (1, 3000), (0, 3000), (3, 2999)]
_CHECKED = set()


def _setup(device, P=3000, deg=3):
    """test_train_step.py's scene (seed 4), and once per P the check that its view shows bare sky
    and splats (about 14 % of the pixels have alpha == 0 and 10 % alpha > 0.5)."""
    cam = gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(P, 3, cam=cam, seed=4)
    settings = gs_scenes.raster_settings_for(cam, deg, device=device)
    gt = torch.rand((3, H, W), generator=torch.Generator().manual_seed(9)).to(device)
    if P not in _CHECKED:
        from diff_gaussian_rasterization import GaussianRasterizer

        d = sc.to(device)
        with torch.no_grad():
            alpha = GaussianRasterizer(settings)(means3D=d.means3D, means2D=torch.zeros_like(d.means3D),
                                                 opacities=d.opacities, shs=d.shs, scales=d.scales,
                                                 rotations=d.rotations, aux_outputs=True)[3]
        assert bool((alpha == 0).any()) and bool((alpha > 0.5).any()), "the scene must show bare sky and splats"
        _CHECKED.add(P)
    return sc, settings, gt


def _texture(device):
    return torch.rand((3, 16, 32), generator=torch.Generator().manual_seed(21)).to(device)


def _prior(device):
    """A positive inverse-depth prior (the scene's depths are 2 .. 10)."""
    return (0.1 + 0.4 * torch.rand((1, H, W), generator=torch.Generator().manual_seed(22))).to(device)


def _model(sc, device, fused=True, sky=True):
    import gs_sky
    import gs_train_step as ts

    m = ts.TrainModel(sc, device, fused=fused)
    if sky:
        s = gs_sky.SkySphere(16, 32).to(device)
        with torch.no_grad():
            s.texture.copy_(_texture(device))
        assert m.attach_sky(s) is s and m.sky is s
        (g,) = m.sky_optimizer.param_groups
        assert type(m.sky_optimizer) is type(m.optimizer) and g["name"] == "sky" and g["eps"] == 1e-15
        assert g["lr"] == ts.FEATURE_LR and g["params"][0] is s.texture
        assert len(m.optimizer.param_groups) == 6  # densify_and_prune's groups: the Gaussians' only
    return m


def _opt_state(opt):
    out, steps = [], []
    for grp in opt.param_groups:
        p = grp["params"][0]
        st = opt.state[p]
        out += [p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
        steps.append(float(st["step"]))
    return out, steps


def _run_pair(device, monkeypatch, active_degree, P, sky, depth, want_aux):
    """Three iterations with loss_item=True, fuse_adam False against True; everything bit-identical.
    want_aux: which of (dL/dinvdepth, dL/dalpha) the fused run's per-tile half must receive."""
    import gs_train
    import gs_train_step as ts
    from diff_gaussian_rasterization import _C

    sc, settings, gt = _setup(device, P=P)
    settings = settings._replace(sh_degree=active_degree)
    kw = dict(sky=True) if sky else {}
    if depth:
        kw.update(depth_prior=_prior(device), depth_weight=0.1)
    runs = []
    for fuse in (False, True):
        m = _model(sc, device, sky=sky)
        seen = []
        if fuse:  # no fall-back to the unfused update or to the statistics' own launch
            def refuse(*a, **k):
                raise AssertionError("fused step fell back to the unfused path")
            monkeypatch.setattr(gs_train.FusedAdam, "step_activated", refuse)
            monkeypatch.setattr(gs_train, "densify_stats", refuse)
            orig = _C.backward_render

            def spy(*a, **k):
                seen.append(k.get("aux_grads"))
                return orig(*a, **k)
            monkeypatch.setattr(_C, "backward_render", spy)
        losses = [ts.train_step(m, settings, gt, loss_item=True, fuse_adam=fuse, **kw) for _ in range(3)]
        torch.cuda.synchronize()
        monkeypatch.undo()
        if fuse:
            assert len(seen) == 3
            for aux in seen:
                assert aux is not None and tuple(g is not None for g in aux) == want_aux
                assert all(g is None or tuple(g.shape) == (1, H, W) for g in aux)
        stats = [t.clone() for t in (m.max_radii2D, m.xyz_gradient_accum, m.denom)]
        runs.append((losses, _opt_state(m.optimizer), stats, _opt_state(m.sky_optimizer) if sky else None, m))
    (la, (sa, ta), da, ka, ma), (lb, (sb, tb), db, kb, mb) = runs
    assert la == lb and ta == tb == [3.0] * 6
    for k, (a, b) in enumerate(zip(sa, sb)):
        assert torch.equal(a, b), k
    for a, b in zip(da, db):
        assert torch.equal(a, b)
    assert mb.denom.sum() > 0
    if sky:
        assert ka[1] == kb[1] == [3.0]
        for k, (a, b) in enumerate(zip(ka[0], kb[0])):
            assert torch.equal(a, b), ("sky", k)
        assert not torch.equal(kb[0][0], _texture(device))
        assert mb.sky.texture.grad is None and ma.sky.texture.grad is None
    for name in NAMES:
        assert getattr(mb, name).grad is None, name
    return ma, mb


@pytest.mark.parametrize("active_degree,P", PARAMS)
def test_fused_adam_equals_unfused_with_sky(device, monkeypatch, active_degree, P):
    """1. The sky behind the splats: the six parameters, both moments, the step counts, the three
    statistics, the texture with its moments and step count and the loss.item() values, bit for bit;
    the fused run's per-tile half received the alpha gradient (and no inverse-depth gradient)."""
    _run_pair(device, monkeypatch, active_degree, P, sky=True, depth=False, want_aux=(False, True))


@pytest.mark.parametrize("active_degree,P", PARAMS)
def test_fused_adam_equals_unfused_with_sky_and_depth_prior(device, monkeypatch, active_degree, P):
    """2. The same with depth_weight = 0.1 and a positive prior: both aux gradients are present and
    the depth chain moves xyz (every depth-chain instantiation of the fused kernel runs)."""
    import gs_train_step as ts

    _run_pair(device, monkeypatch, active_degree, P, sky=True, depth=True, want_aux=(True, True))
    # not vacuous: after one unfused step the prior has moved xyz, and the texture has left its start
    sc, settings, gt = _setup(device, P=P)
    settings = settings._replace(sh_degree=active_degree)
    with_prior, without = _model(sc, device), _model(sc, device)
    ts.train_step(with_prior, settings, gt, loss_item=True, sky=True, depth_prior=_prior(device), depth_weight=0.1)
    ts.train_step(without, settings, gt, loss_item=True, sky=True, depth_prior=_prior(device), depth_weight=0.0)
    assert not torch.equal(with_prior._xyz, without._xyz)
    assert not torch.equal(with_prior.sky.texture.detach(), _texture(device))


def test_fused_adam_equals_unfused_with_depth_prior_only(device, monkeypatch):
    """3. A depth prior without a sky (bg zero): only the inverse-depth gradient reaches the backward."""
    ma, mb = _run_pair(device, monkeypatch, 3, 3000, sky=False, depth=True, want_aux=(True, False))
    assert ma.sky is None and mb.sky_optimizer is None


def test_fused_glue_matches_torch_glue_with_sky_and_depth_prior(device):
    """4. fused=True against fused=False (torch glue around the same rasterizer and sky kernels) with
    sky and depth prior, in test_fused_train_step_matches_torch_glue's bounds: losses at rtol 1e-5,
    max_radii2D and denom equal, the gradient-norm sums at rtol 1e-5, every parameter (the texture with
    its learning rate too) within 2 Adam steps of its learning rate per iteration and >= 99 % of the
    entries equal at 1e-6 relative + 1e-7."""
    import gs_train_step as ts

    sc, settings, gt = _setup(device)
    prior = _prior(device)
    runs = {}
    for fused in (True, False):
        m = _model(sc, device, fused=fused)
        losses = [ts.train_step(m, settings, gt, fused=fused, sky=True, depth_prior=prior, depth_weight=0.1).item()
                  for _ in range(3)]
        torch.cuda.synchronize()
        runs[fused] = (m, losses)
    (mf, lf), (mt, lt) = runs[True], runs[False]
    print("losses fused", lf, "torch glue", lt)
    np.testing.assert_allclose(lf, lt, rtol=1e-5)
    np.testing.assert_array_equal(mf.max_radii2D.cpu().numpy(), mt.max_radii2D.cpu().numpy())
    np.testing.assert_array_equal(mf.denom.cpu().numpy(), mt.denom.cpu().numpy())
    np.testing.assert_allclose(mf.xyz_gradient_accum.cpu().numpy(), mt.xyz_gradient_accum.cpu().numpy(),
                               rtol=1e-5, atol=1e-9)
    pairs = [(n, lr, getattr(mf, n), getattr(mt, n)) for n, lr in zip(
        NAMES, (ts.POSITION_LR_INIT, ts.FEATURE_LR, ts.FEATURE_LR / 20, ts.OPACITY_LR, ts.SCALING_LR, ts.ROTATION_LR))]
    pairs.append(("sky.texture", ts.FEATURE_LR, mf.sky.texture, mt.sky.texture))
    for name, lr, a, b in pairs:
        a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
        d = np.abs(a - b)
        close = d <= 1e-6 * np.abs(b) + 1e-7
        print(f"{name}: max |d| {d.max():.3e}, {close.mean():.4f} of the entries agree")
        assert d.max() <= 2 * 3 * lr + 1e-6, f"{name}: max |d| {d.max():.3e}"
        assert close.mean() >= 0.99, f"{name}: only {close.mean():.4f} of the entries agree"
    assert not torch.equal(mf.sky.texture.detach(), _texture(device))


class _Recorder:
    """A deferring gradient owner that opts in to aux gradients and only records."""
    defers = True
    accepts_aux = True

    def __init__(self):
        self.views = []

    def claim(self, t):
        return None

    def defer_view(self, ctx, inputs, view):
        self.views.append((inputs, view))


def test_protocol_hands_the_inverse_depth_sums_to_an_owner_that_accepts_aux(device):
    """5. One defer_view with inputs["invdepth_sums"] [P] fp32 for a backward with aux gradients, the
    screen-space gradient of the non-deferred aux backward bit for bit; None for a colour-only one."""
    from diff_gaussian_rasterization import GaussianRasterizer, register_gradient_sink, unregister_gradient_sink

    sc, settings, _ = _setup(device)
    d = sc.to(device)
    P = d.means3D.shape[0]
    gen = torch.Generator().manual_seed(5)
    g_col = (1e-3 * torch.randn((3, H, W), generator=gen)).to(device)
    g_inv = (1e-3 * torch.randn((1, H, W), generator=gen)).to(device)
    g_alpha = (1e-3 * torch.randn((1, H, W), generator=gen)).to(device)

    def run(owner, aux):
        leaves = [t.clone().requires_grad_(True) for t in (d.means3D, d.shs, d.opacities, d.scales, d.rotations)]
        m2 = torch.zeros_like(leaves[0], requires_grad=True)
        if owner is not None:
            for t in leaves:
                register_gradient_sink(t, owner)
        try:
            out = GaussianRasterizer(settings)(means3D=leaves[0], means2D=m2, shs=leaves[1], opacities=leaves[2],
                                               scales=leaves[3], rotations=leaves[4], aux_outputs=True)
            loss = (out[0] * g_col).sum()
            if aux:
                loss = loss + (out[2] * g_inv).sum() + (out[3] * g_alpha).sum()
            loss.backward()
        finally:
            for t in leaves:
                unregister_gradient_sink(t)
        torch.cuda.synchronize()
        return leaves, m2

    ref_leaves, ref_m2 = run(None, True)
    assert ref_leaves[0].grad is not None
    owner = _Recorder()
    leaves, m2 = run(owner, True)
    assert len(owner.views) == 1
    inputs, view = owner.views[0]
    sums = inputs["invdepth_sums"]
    assert tuple(sums.shape) == (P,) and sums.dtype == torch.float32 and sums.device == d.means3D.device
    assert inputs["means3D"] is not None and len(view) == 8
    assert torch.equal(m2.grad, ref_m2.grad) and m2.grad.abs().sum() > 0
    assert all(t.grad is None for t in leaves)  # the per-Gaussian half is the owner's
    _, m2p = run(owner, False)  # colour only, through the same owner
    assert len(owner.views) == 2 and "invdepth_sums" in owner.views[1][0]
    assert owner.views[1][0]["invdepth_sums"] is None and m2p.grad is not None


def test_refusals_raise_before_any_launch(device, monkeypatch):
    """6. sky= with a nonzero bg, and sky= or depth_prior= with binning_capacity=: ValueError, and
    neither the render nor the sky is reached."""
    import gs_sky
    import gs_train_step as ts

    sc, settings, gt = _setup(device)
    m = _model(sc, device)
    def params():
        return [getattr(m, n).detach().clone() for n in NAMES] + [m.sky.texture.detach().clone()]
    before = params()

    def refuse(*a, **k):
        raise AssertionError("a refused train_step reached a launch")
    monkeypatch.setattr(ts, "render", refuse)
    monkeypatch.setattr(gs_sky, "compose", refuse)
    lit = settings._replace(bg=torch.tensor([0.0, 0.25, 0.0], device=device))
    for fuse in (False, True):
        with pytest.raises(ValueError, match="settings.bg must be all zeros"):
            ts.train_step(m, lit, gt, loss_item=True, fuse_adam=fuse, sky=True)
        with pytest.raises(ValueError, match="binning_capacity"):
            ts.train_step(m, settings, gt, loss_item=True, fuse_adam=fuse, sky=True, binning_capacity=1 << 16)
        with pytest.raises(ValueError, match="binning_capacity"):
            ts.train_step(m, settings, gt, loss_item=True, fuse_adam=fuse, depth_prior=_prior(device),
                          depth_weight=0.1, binning_capacity=1 << 16)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, params()))
    assert not m.sky_optimizer.state[m.sky.texture] and not m.optimizer.state[m._xyz]  # never stepped


def _full_snapshot(m):
    torch.cuda.synchronize()
    out = []
    for opt in (m.optimizer, m.sky_optimizer):
        st = opt.state_dict()["state"]
        moments = {(i, k): v.clone() for i, s in st.items() for k, v in s.items() if torch.is_tensor(v) and v.dim()}
        steps = {(i, k): float(v) for i, s in st.items() for k, v in s.items() if not torch.is_tensor(v) or not v.dim()}
        out.append((moments, steps))
    tensors = {n: getattr(m, n).detach().clone() for n in NAMES}
    tensors["sky.texture"] = m.sky.texture.detach().clone()
    return tensors, out, [t.clone() for t in (m.max_radii2D, m.xyz_gradient_accum, m.denom)]


def _assert_same_snapshot(before, after):
    for n in before[0]:
        assert torch.equal(before[0][n], after[0][n]), n
    for (bm, bs), (am, as_) in zip(before[1], after[1]):
        assert bm.keys() == am.keys() and bs == as_
        for k in bm:
            assert torch.equal(bm[k], am[k]), k
    for x, y in zip(before[2], after[2]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("fuse_adam", [True, False])
def test_invalid_view_raises_in_its_own_step_with_the_sky_untouched(device, fuse_adam):
    """7. The handled look-back timeout of test_lookback_timeout_raises_in_its_own_step_with_state_untouched
    (gs_debug_set_scan_spin_limit(0): a status flag, every kernel completes) with the sky attached and
    a depth prior: the step raises in its own iteration with parameters, moments, step counts,
    statistics, the texture, its moments and its step count unchanged and its .grad cleared; the next
    two steps equal a model that never saw the failure."""
    import gs_train_step as ts
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    sc, settings, gt = _setup(device)
    kw = dict(loss_item=True, fuse_adam=fuse_adam, sky=True, depth_prior=_prior(device), depth_weight=0.1)
    a, b = _model(sc, device), _model(sc, device)
    ts.train_step(a, settings, gt, **kw)
    ts.train_step(b, settings, gt, **kw)
    before = _full_snapshot(b)
    assert before[1][1][1] and all(v == 1.0 for v in before[1][1][1].values())  # the texture's step count
    prev = lib.gs_debug_set_scan_spin_limit(0)
    try:
        with pytest.raises(RuntimeError, match="look-back wait"):
            ts.train_step(b, settings, gt, **kw)
    finally:
        lib.gs_debug_set_scan_spin_limit(prev)
    _assert_same_snapshot(before, _full_snapshot(b))
    assert b.sky.texture.grad is None
    for _ in range(2):
        assert ts.train_step(a, settings, gt, **kw) == ts.train_step(b, settings, gt, **kw)
    _assert_same_snapshot(_full_snapshot(a), _full_snapshot(b))


def test_timing_record_sky_train_step_1080p(device):
    """8. train_step(sky=True, loss_item=True) with fuse_adam True and False at 1920 x 1080, 1M
    Gaussians, SH3 (bench.py's C3 scene and target), a 512 x 1024 texture: mean of 50 steps after 5
    warm-up steps.  Recorded (GS_SKY_TRAIN_TIMING names a file to keep it in), not asserted."""
    import time

    import gs_sky
    import gs_train_step as ts

    cam = gs_scenes.identity_camera(1920, 1080)
    sc = gs_scenes.random_gaussians(1_000_000, 3, cam=cam, seed=0)
    settings = gs_scenes.raster_settings_for(cam, 3, device=device)
    gt = torch.rand((3, 1080, 1920), generator=torch.Generator().manual_seed(2)).to(device)
    lines = ["train_step(sky=True, loss_item=True), C3 (1M Gaussians SH3 1920x1080), texture 512x1024, mean of 50:"]
    for fuse in (True, False):
        m = ts.TrainModel(sc, device, fused=True)
        m.attach_sky(gs_sky.SkySphere(512, 1024).to(device))
        for _ in range(5):
            ts.train_step(m, settings, gt, loss_item=True, fuse_adam=fuse, sky=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(50):
            loss = ts.train_step(m, settings, gt, loss_item=True, fuse_adam=fuse, sky=True)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) / 50
        assert np.isfinite(loss) and torch.isfinite(m.sky.texture).all()
        lines.append(f"fuse_adam={fuse}: {1e3 * dt:.4f} ms/iter, {1.0 / dt:.2f} it/s")
        del m
    text = "\n".join(lines) + "\n"
    print(text)
    if os.environ.get("GS_SKY_TRAIN_TIMING"):
        with open(os.environ["GS_SKY_TRAIN_TIMING"], "w") as f:
            f.write(text)
