"""The fused per-Gaussian backward + Adam step (k_preprocess_bwd_adam<DEG, AUX>, csrc/gs_backward.hip; the
entries gs_backward_gaussians_adam / _adam_stats / _adam_stats_aux) at row, group and visibility edges.

The kernel is driven through the pieces train_step(fuse_adam=True) uses -- render() with an _AdamBackward
owner, (image * dpix).sum().backward(), FusedAdam.step_fused_backward -- so dL/dpix is the test's own and the
loss kernels are not in the chain.  Scenes, pokes, hyper-parameters and the fp64 reference:
tests/fused_adam_cases.py (their properties: tests/test_fused_adam_cases.py).  What is compared:

  a. with the unfused step (render, add_densification_stats, FusedAdam.step_activated), bit for bit, at every
     row-count edge and active degree, three steps through three cameras of different image sizes after
     poke_raw; rows without instances keep zero moments / decay them exactly; coefficients past the active
     degree are never touched
  b. per-group weight decay, step count, betas, eps and maximize: with the unfused step bit for bit, and with
     torch.optim.Adam (fed the raw gradients of plain autograd) at test_train_updates.py's tolerances
  c. the first step from zero moments with the fp64 dense reference: exp_avg / (1 - b1) is the raw gradient
     the kernel formed; bounds of tests/test_gpu_dense.py per tensor; the parameter moved by -lr sign(ref)
  d. the aux variant (a depth prior) through train_step, and by pieces with the inverse-depth sums of rows
     without instances overwritten (they are unspecified there and must not be read)
"""
import numpy as np
import pytest
import torch

import fused_adam_cases as fac
import gs_scenes
from test_train_updates import P_TOL, S_TOL

pytestmark = pytest.mark.gpu

NAMES = fac.NAMES
STATS = ("max_radii2D", "xyz_gradient_accum", "denom")


def _params(m):
    return [getattr(m, n) for n in NAMES]


def _snapshot(m):
    """{name: (parameter, exp_avg, exp_avg_sq)} as clones (zero moments before the first step), the step
    counts and the densification statistics."""
    out = {}
    steps = []
    for n, p in zip(NAMES, _params(m)):
        st = m.optimizer.state.get(p, {})
        z = torch.zeros_like(p)
        out[n] = (p.detach().clone(), st["exp_avg"].clone() if st else z, st["exp_avg_sq"].clone() if st else z.clone())
        steps.append(float(st["step"]) if st else 0.0)
    out["steps"] = steps
    out["stats"] = [getattr(m, s).clone() for s in STATS]
    return out


def _assert_same(a, b, what=""):
    assert a["steps"] == b["steps"], (what, a["steps"], b["steps"])
    for n in NAMES:
        for k, (x, y) in enumerate(zip(a[n], b[n])):
            assert torch.equal(x, y), (what, n, ("param", "exp_avg", "exp_avg_sq")[k],
                                       int((x != y).sum()), float((x - y).abs().max()))
    for s, x, y in zip(STATS, a["stats"], b["stats"]):
        assert torch.equal(x, y), (what, s)


def _opacity(m):
    return torch.sigmoid(m._opacity.detach()).cpu().numpy()


def _step(ts, gs_train, m, settings, dpix, fuse, stats=True, dinv=None, poison=None):
    """One step by pieces; returns the view's radii.  dinv: the aux render, with dL/dinvdepth = dinv.
    poison(inputs["invdepth_sums"], radii): called before the fused launch."""
    aux = dinv is not None
    acts = []
    owner = ts._AdamBackward() if fuse else None
    try:
        out = ts.render(m, settings, True, acts, True, None, owner, aux_outputs=aux)
        image, viewspace, radii = out[0], out[1], out[2]
        loss = (image * dpix).sum()
        if aux:
            loss = loss + (out[3] * dinv).sum()
        loss.backward()
        with torch.no_grad():
            if fuse:
                assert owner.pending is not None, "the rasterizer did not defer its per-Gaussian half"
                inputs, view = owner.pending
                owner.pending = None
                assert (inputs.get("invdepth_sums") is not None) == aux
                if poison is not None:
                    poison(inputs["invdepth_sums"], radii)
                st = (m.max_radii2D, m.xyz_gradient_accum, m.denom, radii, viewspace.grad) if stats else None
                m.optimizer.step_fused_backward(_params(m), inputs, view, st)
                assert all(p.grad is None for p in _params(m))
            else:
                if stats:
                    gs_train.add_densification_stats(m, viewspace, radii)
                shs, opac, scales, rots = acts
                m.optimizer.step_activated(
                    {m._features_dc: ("features_dc", shs.grad), m._features_rest: ("features_rest", shs.grad),
                     m._opacity: ("sigmoid", opac.grad), m._scaling: ("exp", scales.grad),
                     m._rotation: ("normalize", rots.grad)}, sh_coeffs=shs.shape[1])
            m.optimizer.zero_grad(set_to_none=True)
    finally:
        if owner is not None:
            owner.disarm()
    return radii


def _decayed(m1, v1, b1, b2):
    """The moments of a zero gradient (adam_update, torch's lerp / mul): exp_avg + (1 - b1)(0 - exp_avg) as
    one fused multiply-add -- exact in float64 (a 24-bit by 24-bit product plus a 24-bit term a few binades
    up), rounded once to float32 -- and exp_avg_sq * b2 in float32."""
    w1 = torch.tensor(1.0 - b1, dtype=torch.float64).float().double()
    m = (m1.double() - w1 * m1.double()).float()
    v = v1 * torch.tensor(b2, dtype=torch.float64).float().to(v1.device)
    return m, v


def _assert_decayed(before, after, rows, b1=0.9, b2=0.999, names=NAMES, what=""):
    """Rows without instances in a step: moments of `before` multiplied by b1 / b2 exactly as float32 does
    it, and a parameter that moves wherever its exp_avg is not (nearly) zero."""
    rows = torch.from_numpy(rows).to(before[names[0]][0].device)
    for n in names:
        (p0, m0, v0), (p1, m1, v1) = before[n], after[n]
        em, ev = _decayed(m0[rows], v0[rows], b1, b2)
        assert torch.equal(m1[rows], em), (what, n, "exp_avg")
        assert torch.equal(v1[rows], ev), (what, n, "exp_avg_sq")
        torch.testing.assert_close(m1[rows], m0[rows] * b1, rtol=2.0 ** -22, atol=1e-37)
        live = m0[rows].abs() > 1e-10
        assert bool(((p1[rows] != p0[rows]) | ~live).all()), (what, n, "the parameter did not move")


CASES_A = [(P, 3) for P in fac.P_EDGES] + [(P, d) for P in (257, 352) for d in (0, 1, 2)]


@pytest.mark.parametrize("P,deg", CASES_A, ids=[f"P{P}-deg{d}" for P, d in CASES_A])
def test_bit_equal_unfused_at_row_edges(device, P, deg):
    """a. Three steps with cameras 0, 1, 2 after poke_raw.  The last workgroup holds 1, 2, 3, 4, 255, 256,
    1, 2, 3 or 96 rows: every tail of adam_sh_block for both SH tensors, one and two workgroups."""
    import gs_train
    import gs_train_step as ts

    sc, cams = fac.model_scene(P)
    runs = {}
    for fuse in (False, True):
        m = ts.TrainModel(sc, device, fused=True)
        poked = fac.poke_raw(m)
        snaps, seens, rads = [_snapshot(m)], [], []
        for v, cam in enumerate(cams):
            settings = gs_scenes.raster_settings_for(cam, deg, device=device)
            op = _opacity(m)
            radii = _step(ts, gs_train, m, settings, fac.dpix_for(v, cam).to(device), fuse)
            seens.append(fac.seen(radii.cpu().numpy(), op))
            rads.append((radii > 0).cpu())
            snaps.append(_snapshot(m))
        torch.cuda.synchronize()
        runs[fuse] = (snaps, seens, poked)
    (sa, va, _), (sb, vb, poked) = runs[False], runs[True]
    for k in range(4):
        _assert_same(sa[k], sb[k], f"after step {k}")
    assert sb[3]["steps"] == [3.0] * 6
    assert all(np.array_equal(x, y) for x, y in zip(va, vb))
    for n in NAMES:
        assert all(bool(torch.isfinite(t).all()) for t in sb[3][n]), n
    if ("_opacity", -15.0) in poked:
        assert not any(s[poked[("_opacity", -15.0)]] for s in vb)
    for (name, what), i in poked.items():  # the other poked rows are still rendered
        if what != -15.0:
            assert vb[0][i], (name, what)
    # rows without instances in step 1: zero moments, the parameter as it was
    s0, s1, s2 = sb[0], sb[1], sb[2]
    inv = torch.from_numpy(~vb[0]).to(device)
    vis = torch.from_numpy(vb[0]).to(device)
    for n in NAMES:
        (p0, _, _), (p1, m1, v1) = s0[n], s1[n]
        assert not m1[inv].any() and not v1[inv].any() and torch.equal(p1[inv], p0[inv]), n
        some = vis.clone()
        if n == "_rotation":  # R(q) is quadratic in q: the zero quaternion's own gradient is zero
            some[poked[("_rotation", "zero")]] = False
        if some.any() and not (n == "_features_rest" and deg == 0):
            assert m1[some].any() and v1[some].any() and not torch.equal(p1[some], p0[some]), n
    # seen in step 1, not in step 2: moments times b1 / b2, and the parameter still moves
    gone = vb[0] & ~vb[1]
    if P >= 255:
        assert gone.sum() >= 16 and (~vb[0]).sum() >= 16
    names = [n for n in NAMES if not (n == "_features_rest" and deg == 0)]
    _assert_decayed(s1, s2, ~vb[1], names=names, what="step 2")
    _assert_decayed(s2, sb[3], ~vb[2], names=names, what="step 3")
    # coefficients past the active degree: never touched
    k = (deg + 1) ** 2 - 1
    for s in sb[1:]:
        p, m1, v1 = s["_features_rest"]
        assert not m1[:, k:].any() and not v1[:, k:].any() and torch.equal(p[:, k:], s0["_features_rest"][0][:, k:])
    # the statistics counted every row with a radius, once per step
    assert torch.equal(sb[3]["stats"][2].reshape(-1).cpu(), sum(r.float() for r in rads))


CASES_B = [(mx, hy, st) for mx in (False, True) for hy in ("default", "odd") for st in (True, False)]


@pytest.mark.parametrize("maximize,hyper,stats", CASES_B,
                         ids=[f"{'max' if a else 'min'}-{b}-{'stats' if c else 'nostats'}" for a, b, c in CASES_B])
def test_per_group_hyper_parameters(device, maximize, hyper, stats):
    """b. odd_hyper at P = 259: a weight decay and a step count of its own per group (the kernel indexes
    nss / bc2s / wd by group at seven places), non-zero moments to start from; two steps, cameras 0 and 1.
    Fused against unfused bit for bit; fused against torch.optim.Adam on the raw gradients of plain
    autograd (gs_train.activate in front of the rasterizer) at P_TOL / S_TOL."""
    import gs_train
    import gs_train_step as ts

    P = 259
    sc, cams = fac.model_scene(P)
    kw = dict(maximize=maximize)
    if hyper == "default":
        kw.update(betas=(0.9, 0.999), eps=1e-15)
    snaps, seens = {}, []
    for kind in ("unfused", "fused", "torch"):
        m = ts.TrainModel(sc, device, fused=kind != "torch")
        assert isinstance(m.optimizer, torch.optim.Adam if kind == "torch" else gs_train.FusedAdam)
        fac.odd_hyper(m.optimizer, **kw)
        hist = [_snapshot(m)]
        for v in (0, 1):
            cam = cams[v]
            settings = gs_scenes.raster_settings_for(cam, 3, device=device)
            dpix = fac.dpix_for(v, cam).to(device)
            op = _opacity(m)
            if kind == "torch":
                image, _, radii = ts.render(m, settings, fused=True)
                (image * dpix).sum().backward()
                m.optimizer.step()
                m.optimizer.zero_grad(set_to_none=True)
            else:
                radii = _step(ts, gs_train, m, settings, dpix, kind == "fused", stats=stats)
            if kind == "fused":
                seens.append(fac.seen(radii.cpu().numpy(), op))
            hist.append(_snapshot(m))
        torch.cuda.synchronize()
        snaps[kind] = hist
    for k in range(3):
        _assert_same(snaps["unfused"][k], snaps["fused"][k], f"after step {k}")
    fused, ref = snaps["fused"][2], snaps["torch"][2]
    assert fused["steps"] == ref["steps"] == [float(s + 2) for s in fac.STEPS]
    assert seens[0].any() and not seens[0].all() and (seens[0] & ~seens[1]).any()
    if stats:
        assert float(fused["stats"][2].sum()) >= float(seens[0].sum() + seens[1].sum())
    else:
        assert not any(bool(t.any()) for t in fused["stats"])
    for n in NAMES:
        (p, m1, v1), (rp, rm, rv) = fused[n], ref[n]
        assert not torch.equal(p, snaps["fused"][0][n][0]), n
        torch.testing.assert_close(p, rp, **P_TOL)
        torch.testing.assert_close(m1, rm, **S_TOL)
        torch.testing.assert_close(v1, rv, **S_TOL)
    # (rows without instances have no gradient but their group's weight decay, g = wd * p: torch's Adam above
    # is the reference for them too)


@pytest.mark.parametrize("deg", [3, 1])
@pytest.mark.parametrize("v", [0, 1, 2])
def test_first_step_against_fp64_reference(device, v, deg):
    """c. P = 352, zero moments, weight_decay 0: exp_avg = (1 - b1) g and exp_avg_sq = (1 - b2) g^2, so
    g = exp_avg / (1 - b1) is the raw-parameter gradient the kernel formed.  Compared with the fp64 dense
    reference behind torch's activations (fused_adam_cases.ref_forward), tests/test_gpu_dense.py's
    procedure (flagged pixels masked out of dpix, rows whose fp32 radius differs left out: at most one)
    and bounds, per tensor: 1e-5 |ref| + 1e-5 max|ref| for opacity and SH, 1e-5 |ref| + 5e-5 max|ref| for xyz,
    scaling and rotation; exp_avg_sq against (1 - b2) ref^2 at twice that.  Where |ref| exceeds its bound the
    parameter moved by -lr sign(ref) to within 2^-22 (|p| + lr); elements inside the bound (at most 5 % of
    the visible rows' elements, non-zero ones) are left out of that sign check only; elements whose
    reference gradient is exactly zero (a clamped colour channel) keep zero moments and do not move."""
    import gs_train
    import gs_train_step as ts

    sc, cams = fac.model_scene(352)
    cam = cams[v]
    m = ts.TrainModel(sc, device, fused=True)
    settings = gs_scenes.raster_settings_for(cam, deg, device=device)
    raw = [p.detach().clone() for p in _params(m)]
    op = _opacity(m)
    leaves, rimg, rradii, flag = fac.ref_forward(raw, cam, deg, device)
    rects = fac.ref_rects(raw, cam, deg, device)
    b1, b2 = m.optimizer.param_groups[0]["betas"]
    w1 = float(torch.tensor(1.0 - b1, dtype=torch.float64).float())
    w2 = float(torch.tensor(1.0 - b2, dtype=torch.float64).float())

    acts = []
    owner = ts._AdamBackward()
    try:
        image, viewspace, radii = ts.render(m, settings, True, acts, True, None, owner)
        rdiff = (radii.cpu() != rradii.cpu()).numpy()
        assert rdiff.sum() <= 1, f"{int(rdiff.sum())} radii differ"
        fl = fac.widen_flags(flag.cpu().numpy().copy(), rects, rdiff)
        print(f"\n[fused adam, view {v}, degree {deg}] flagged pixels {int(fl.sum())}/{fl.size}, radii differing "
              f"{int(rdiff.sum())}/352")
        assert fl.mean() <= 0.02
        dpm = fac.dpix_for(v, cam).to(device) * torch.from_numpy(~fl).to(device)[None]
        (image * dpm).sum().backward()
        (rimg * dpm.double()).sum().backward()
        with torch.no_grad():
            inputs, view = owner.pending
            owner.pending = None
            m.optimizer.step_fused_backward(
                _params(m), inputs, view, (m.max_radii2D, m.xyz_gradient_accum, m.denom, radii, viewspace.grad))
    finally:
        owner.disarm()
    torch.cuda.synchronize()
    keep = ~rdiff
    visible = fac.seen(rradii.cpu().numpy(), op)[keep]
    assert visible.sum() >= 128
    for k, (n, p, leaf) in enumerate(zip(NAMES, _params(m), leaves)):
        st = m.optimizer.state[p]
        lr = float(m.optimizer.param_groups[k]["lr"])
        ref = leaf.grad.cpu().numpy()[keep]
        got = st["exp_avg"].double().cpu().numpy()[keep] / w1
        got_v = st["exp_avg_sq"].double().cpu().numpy()[keep]
        p0, p1 = raw[k].double().cpu().numpy()[keep], p.detach().double().cpu().numpy()[keep]
        bnd = fac.bound(n, ref)
        d = np.abs(got - ref)
        R = w2 * ref * ref
        tol_v = 2.0 * (fac.RTOL * np.abs(R) + fac.BOUND_FRAC[n] * float(np.abs(R).max(initial=0.0)))
        dv = np.abs(got_v - R)
        decided = np.abs(ref) > bnd
        dev = np.abs((p1 - p0) + lr * np.sign(ref))
        tol_p = 2.0 ** -22 * (np.abs(p0) + lr)
        share, zeros, count = fac.inside_share(n, ref, visible, deg)
        print(f"  {n}: max|g - ref| {d.max():.3e} = {float((d / np.maximum(bnd, 1e-300)).max()):.3f} of its bound "
              f"({d.max() / np.abs(ref).max():.2e} of max|ref| {np.abs(ref).max():.3e}); exp_avg_sq "
              f"{float((dv / np.maximum(tol_v, 1e-300)).max()):.3f} of its bound; step deviation "
              f"{float((dev / tol_p)[decided].max(initial=0.0)):.3f} of 2^-22 (|p| + lr) over {int(decided.sum())} "
              f"elements; {share:.4f} of {count} inside the bound, {zeros} exact zeros")
        assert (d <= bnd).all(), f"{n}: {int((d > bnd).sum())}/{d.size} gradients beyond the bound"
        assert (dv <= tol_v).all(), f"{n}: {int((dv > tol_v).sum())}/{dv.size} of exp_avg_sq beyond the bound"
        assert (dev[decided] <= tol_p[decided]).all(), \
            f"{n}: {int((dev[decided] > tol_p[decided]).sum())} parameters did not move by -lr sign(ref)"
        assert share <= 0.05, (n, share)
        zero = ref == 0
        assert not got[zero].any() and not got_v[zero].any() and np.array_equal(p1[zero], p0[zero]), n
        assert decided[visible].any(), n


def _prior(cam, seed, device):
    """A positive inverse-depth prior (the scene's depths are 0.25 .. 4)."""
    g = torch.Generator().manual_seed(seed)
    return (0.2 + 2.0 * torch.rand((1, cam.image_height, cam.image_width), generator=g)).to(device)


@pytest.mark.parametrize("P", [257, 352])
def test_aux_variant_through_train_step(device, P, monkeypatch):
    """d. train_step(fuse_adam=True / False, depth_prior=, depth_weight=0.1, loss_item=True): three steps, one
    per camera with its own ground truth and prior; losses, parameters, moments, step counts and statistics
    bit-identical.  Rows without instances in a step got no gradient at all, so no depth-chain term either:
    their moments (xyz's among them) decay by exactly b1 / b2."""
    import gs_train
    import gs_train_step as ts

    sc, cams = fac.model_scene(P)
    runs = {}
    for fuse in (False, True):
        m = ts.TrainModel(sc, device, fused=True)
        if fuse:  # no fall-back to the unfused update
            def refuse(*a, **k):
                raise AssertionError("fused step fell back to the unfused path")
            monkeypatch.setattr(gs_train.FusedAdam, "step_activated", refuse)
        snaps, seens, losses = [_snapshot(m)], [], []
        for v, cam in enumerate(cams):
            settings = gs_scenes.raster_settings_for(cam, 3, device=device)
            g = torch.Generator().manual_seed(40 + v)
            gt = torch.rand((3, cam.image_height, cam.image_width), generator=g).to(device)
            with torch.no_grad():
                radii = ts.render(m, settings, fused=True)[2]
            seens.append(fac.seen(radii.cpu().numpy(), _opacity(m)))
            losses.append(ts.train_step(m, settings, gt, loss_item=True, fuse_adam=fuse,
                                        depth_prior=_prior(cam, 50 + v, device), depth_weight=0.1))
            snaps.append(_snapshot(m))
        torch.cuda.synchronize()
        monkeypatch.undo()
        runs[fuse] = (snaps, seens, losses)
    (sa, va, la), (sb, vb, lb) = runs[False], runs[True]
    assert la == lb and all(np.isfinite(x) for x in lb)
    for k in range(4):
        _assert_same(sa[k], sb[k], f"after step {k}")
    assert sb[3]["steps"] == [3.0] * 6 and float(sb[3]["stats"][2].sum()) > 0
    assert (vb[0] & ~vb[1]).sum() >= 16 and ((vb[0] | vb[1]) & ~vb[2]).sum() >= 16
    for k in range(3):
        _assert_decayed(sb[k], sb[k + 1], ~vb[k], what=f"step {k + 1}")
        vis = torch.from_numpy(vb[k]).to(device)
        assert not torch.equal(sb[k]["_xyz"][1][vis], sb[k + 1]["_xyz"][1][vis])


def test_aux_variant_ignores_sums_of_rows_without_instances(device):
    """d. The aux render by pieces, dL/dinvdepth the test's own: the per-tile half writes the inverse-depth
    sums of Gaussians with instances only, the other rows of that buffer are unspecified.  Here they are
    overwritten with 1e6 before the fused launch: everything stays bit-identical to the unfused step
    (k_depth_chain_aux skips those rows), and their xyz moments decay by exactly b1 / b2."""
    import gs_train
    import gs_train_step as ts

    P = 352
    sc, cams = fac.model_scene(P)
    runs = {}
    for fuse in (False, True):
        m = ts.TrainModel(sc, device, fused=True)
        snaps, seens = [_snapshot(m)], []
        for v, cam in enumerate(cams):
            settings = gs_scenes.raster_settings_for(cam, 3, device=device)
            g = torch.Generator().manual_seed(60 + v)
            dinv = torch.randn((1, cam.image_height, cam.image_width), generator=g).to(device)
            op = _opacity(m)
            poisoned = []

            def poison(sums, radii):
                rows = torch.from_numpy(~fac.seen(radii.cpu().numpy(), op)).to(sums.device)
                sums[rows] = 1e6
                poisoned.append(int(rows.sum()))
            radii = _step(ts, gs_train, m, settings, fac.dpix_for(v, cam).to(device), fuse, dinv=dinv,
                          poison=poison if fuse else None)
            assert not fuse or poisoned[0] >= 16
            seens.append(fac.seen(radii.cpu().numpy(), op))
            snaps.append(_snapshot(m))
        torch.cuda.synchronize()
        runs[fuse] = (snaps, seens)
    (sa, va), (sb, vb) = runs[False], runs[True]
    for k in range(4):
        _assert_same(sa[k], sb[k], f"after step {k}")
    for k in range(3):
        _assert_decayed(sb[k], sb[k + 1], ~vb[k], what=f"step {k + 1}")
    # the depth term is in the chain: the same steps without dL/dinvdepth end elsewhere
    m = ts.TrainModel(sc, device, fused=True)
    settings = gs_scenes.raster_settings_for(cams[0], 3, device=device)
    _step(ts, gs_train, m, settings, fac.dpix_for(0, cams[0]).to(device), True)
    assert not torch.equal(m.optimizer.state[m._xyz]["exp_avg"], sb[1]["_xyz"][1])
