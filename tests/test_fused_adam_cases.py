"""The scenes, pokes and image gradients of tests/fused_adam_cases.py have the properties their GPU tests
(tests/test_gpu_fused_adam.py) rely on, by the fp64 dense reference alone (tests/dense_ref.py): conditions on
the inputs, checked without a GPU."""
import numpy as np
import pytest
import torch

import fused_adam_cases as fac
import fused_views_cases as fvc


def _seen_by_camera(P, deg=3):
    sc, cams = fac.model_scene(P)
    leaves = dict(means3D=sc.means3D, opacities=sc.opacities, shs=sc.shs, scales=sc.scales, rotations=sc.rotations)
    op = sc.opacities.numpy()
    return np.stack([fvc.contributes(fvc.dense_prep(leaves, c, deg)["radii"].numpy(), op) for c in cams], 1)  # [P, 3]


def test_p_edges_leave_every_tail_of_both_sh_tensors():
    """The last workgroup's rows: 1, 2, 3, 4, 255, 256, 1, 2, 3, 96.  features_dc (3 floats per row) and
    features_rest (45) then end in every residue mod 4, have a block without any float4 (one row of
    features_dc) and blocks that are float4s only; one-workgroup and two-workgroup grids both occur."""
    last = [P - 256 * ((P - 1) // 256) for P in fac.P_EDGES]
    assert last == [1, 2, 3, 4, 255, 256, 1, 2, 3, 96]
    for W in (3, 45):
        assert {(n * W) % 4 for n in last} == {0, 1, 2, 3}
    assert 1 * 3 // 4 == 0
    assert {(P + 255) // 256 for P in fac.P_EDGES} == {1, 2}


def test_model_scene_is_the_visibility_scene_in_a_fixed_order():
    sc, cams = fac.model_scene(352)
    vis = fvc.visibility_scene()
    rows = fac.model_rows(352)
    assert sorted(rows.tolist()) == list(range(352))
    assert torch.equal(sc.means3D, vis.leaves["means3D"][rows]) and torch.equal(sc.shs, vis.leaves["shs"][rows])
    assert sc.shs.shape == (352, 16, 3) and sc.sh_degree == 3
    assert [(c.image_width, c.image_height) for c in cams] == [(64, 48), (80, 32), (48, 64)]
    for P in fac.P_EDGES:  # every size is a prefix of the same order
        s, _ = fac.model_scene(P)
        assert s.P == P and torch.equal(s.means3D, sc.means3D[:P]) and torch.equal(s.opacities, sc.opacities[:P])
        assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (s.means3D, s.opacities, s.scales,
                                                                             s.rotations, s.shs))
    # past the scene's rows: copies with jitter, not duplicates
    big, _ = fac.model_scene(400)
    assert big.P == 400 and torch.equal(big.means3D[:352], sc.means3D)
    d = (big.means3D[352:] - sc.means3D[:48]).norm(dim=1) / sc.means3D[:48].norm(dim=1)
    assert float(d.max()) <= 1.01e-3 and float(d.min()) > 0
    # the first four rows mix the clusters: the first is seen by every camera
    first = fac.model_groups(4)
    assert first[0] in fac.SEEN_BY_ALL and len(set(first)) == 4, first


def test_the_last_row_of_every_size_is_seen():
    """adam_sh_block's scalar tail holds floats of the last row only (at most 3): that row gets a gradient in
    one of the three steps -- from 255 rows on in the first, from zero moments -- so a tail that is not
    updated shows.  (With 4 and 256 rows there is no tail.)"""
    seen = _seen_by_camera(352)
    for P in fac.P_EDGES:
        assert seen[P - 1].any(), P
        if P >= 255:
            assert seen[P - 1, 0], P


@pytest.mark.parametrize("P", [p for p in fac.P_EDGES if p >= 255])
def test_every_camera_sees_some_rows_and_misses_others(P):
    """Visible and invisible rows under each camera (in the last workgroup too where there are two), some
    row that camera 0 sees and camera 1 does not, one that no camera sees, and the colour-clamp cluster."""
    seen = _seen_by_camera(P)
    for v in range(3):
        assert seen[:, v].sum() >= 16 and (~seen[:, v]).sum() >= 16, (v, seen[:, v].sum())
    assert (seen[:, 0] & ~seen[:, 1]).sum() >= 16 and (seen[:, 1] & ~seen[:, 2]).sum() >= 16
    assert (~seen.any(1)).sum() >= 16 and seen.all(1).sum() >= 16
    groups = fac.model_groups(P)
    assert groups.count("clamp") >= 16
    if P >= 352:
        assert seen[256:].any(0).all() and (~seen[256:]).any(0).all()


def test_small_prefixes_mix_seen_and_unseen_rows():
    """P = 1: a row every camera sees.  From P = 2 on camera 1 and 2 miss a row, from P = 3 on camera 0 does."""
    seen = _seen_by_camera(4)
    assert seen[0].all()
    assert not seen[:2, 1].all() and not seen[:2, 2].all() and seen[:2, 0].all() and not seen[:3, 0].all()
    assert seen.any(1).all()


def test_clamp_cluster_clamps_in_one_view_only():
    sc, cams = fac.model_scene(352)
    leaves = dict(means3D=sc.means3D, shs=sc.shs)
    sel = np.asarray(fac.model_groups(352)) == "clamp"
    for D in (1, 2, 3):
        b1, b2 = fvc.clamp_bits(leaves, cams[1], D)[sel], fvc.clamp_bits(leaves, cams[2], D)[sel]
        assert not b1[:, 0].any() and b2[:, 0].all()


def test_poked_rows_are_seen_by_every_camera():
    """poke_raw's rows: five distinct ones from P = 255 on, each seen by all three cameras before the poke;
    the tiny scenes get the first pokes only (P = 1: the zero quaternion)."""
    for P in fac.P_EDGES:
        rows = fac.poke_rows(P)
        assert len(set(rows)) == len(rows) and all(r < P for r in rows)
        assert len(rows) == (len(fac.POKES) if P >= 255 else 1), (P, rows)
        assert _seen_by_camera(P)[rows].all()
    assert fac.POKES[0] == ("_rotation", "zero") and fac.poke_rows(1) == [0]


def test_poke_raw_writes_the_edges():
    class M:
        pass

    sc, _ = fac.model_scene(259)
    m = M()
    m.P = 259
    for name, t in zip(fac.NAMES, fac.raw_of_scene(sc)):
        setattr(m, name, t.clone())
    before = [getattr(m, n).detach().clone() for n in fac.NAMES]
    done = fac.poke_raw(m)
    assert len(done) == 5
    assert float(m._rotation[done[("_rotation", "zero")]].abs().max()) == 0.0
    tiny = m._rotation[done[("_rotation", 1e-8)]].detach().norm()
    assert 1e-9 < float(tiny) < 1e-7
    assert float(m._opacity[done[("_opacity", 15.0)]]) == 15.0 and float(m._opacity[done[("_opacity", -15.0)]]) == -15.0
    assert (m._scaling[done[("_scaling", -20.0)]] == -20.0).all()
    for n, b in zip(fac.NAMES, before):  # nothing else moved
        changed = (getattr(m, n).detach() != b).reshape(259, -1).any(1)
        assert int(changed.sum()) == sum(1 for (name, _w) in done if name == n), n
    # sigmoid(-15) is below 1/255: that row is no longer rendered; sigmoid(15) rounds below 1 in float32
    lo, hi = (float(torch.sigmoid(torch.tensor(x))) for x in (-15.0, 15.0))
    assert lo < 1.0 / 255.0 < 0.99 < hi < 1.0


def test_odd_hyper_sets_distinct_groups_and_the_same_state_twice():
    def opt():
        ps = [torch.nn.Parameter(torch.zeros(s)) for s in ((7, 3), (7, 1, 3), (7, 15, 3), (7, 1), (7, 3), (7, 4))]
        return torch.optim.Adam([{"params": [p], "lr": 1e-3} for p in ps], lr=0.0, eps=1e-15)

    a, b = opt(), opt()
    fac.odd_hyper(a)
    fac.odd_hyper(b, maximize=True, betas=(0.9, 0.999), eps=1e-15)
    wds = [g["weight_decay"] for g in a.param_groups]
    steps = [float(a.state[g["params"][0]]["step"]) for g in a.param_groups]
    assert len(set(wds)) == 6 and min(wds) > 0 and len(set(steps)) == 6 and min(steps) >= 1
    assert all(g["betas"] == (0.8, 0.99) and g["eps"] == 1e-8 and g["maximize"] is False for g in a.param_groups)
    assert all(g["betas"] == (0.9, 0.999) and g["eps"] == 1e-15 and g["maximize"] is True for g in b.param_groups)
    for ga, gb in zip(a.param_groups, b.param_groups):
        sa, sb = a.state[ga["params"][0]], b.state[gb["params"][0]]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
        assert float(sa["exp_avg"].abs().min()) > 0 and float(sa["exp_avg_sq"].min()) >= 0
        assert sa["step"].dtype == torch.float32 and sa["step"].device.type == "cpu"


@pytest.mark.parametrize("deg", [3, 1])
@pytest.mark.parametrize("v", [0, 1, 2])
def test_reference_gradients_decide_the_first_step(v, deg):
    """The cap of the fp64 comparison, from the reference alone: with dpix_for(v), in every tensor at most
    5 % of the elements of the visible rows have a non-zero reference gradient within its own error bound
    (1e-5 |ref| + frac max|ref|), where the reference does not decide the sign of the first Adam step.
    Elements whose reference gradient is exactly zero (a colour channel clamped at 0: the clamp cluster
    in view 2) are not among them: the GPU test holds those to zero moments and an unmoved parameter.
    Few pixels sit at a decision (tests/test_gpu_dense.py's 2 %)."""
    sc, cams = fac.model_scene(352)
    raw = fac.raw_of_scene(sc)
    leaves, img, radii, flag = fac.ref_forward(raw, cams[v], deg)
    assert float(flag.double().mean()) <= 0.02
    dp = fac.dpix_for(v, cams[v]).double() * (~flag)[None]
    assert 0.0 < float((dp < 0).double().mean()) < 0.1  # mostly of one sign, not all
    (img * dp).sum().backward()
    visible = fac.seen(radii.numpy(), torch.sigmoid(raw[3]).numpy())
    assert np.array_equal(visible, _seen_by_camera(352, deg)[:, v])
    for name, leaf in zip(fac.NAMES, leaves):
        g = leaf.grad.numpy()
        assert np.isfinite(g).all() and not g[~visible].any(), name  # rows without instances: no gradient at all
        share, zeros, n = fac.inside_share(name, g, visible, deg)
        print(f"view {v} degree {deg} {name}: {share:.4f} of {n} inside the bound, {zeros} exact zeros, "
              f"max|ref| {np.abs(g).max():.3e}")
        assert share <= 0.05, (name, share)
        if name in ("_features_dc", "_features_rest"):
            assert zeros <= 0.12 * n, (name, zeros, n)
        else:
            assert zeros == 0, (name, zeros)
        k = fac.active_columns(name, deg)
        if k is not None and k < 15:
            assert not g[:, k:].any()
