"""The constructed scenes of tests/fused_views_cases.py have the properties their GPU tests
(tests/test_gpu_backward_gaussians.py) rely on, by the fp64 dense reference alone (tests/dense_ref.py):
conditions on the inputs, checked without a GPU."""
import math

import numpy as np
import pytest
import torch

import dense_ref
import fused_views_cases as fvc

NAMES = [g[0] for g in fvc.VIS_GROUPS]


@pytest.fixture(scope="module")
def vis():
    return fvc.visibility_scene()


@pytest.fixture(scope="module")
def vis_prep(vis):
    return [fvc.dense_prep(vis.leaves, c, 3) for c in vis.cams]


def _seen(vis, vis_prep):
    op = vis.leaves["opacities"].numpy()
    return np.stack([fvc.contributes(q["radii"].numpy(), op) for q in vis_prep], 1)  # [P, 3]


def test_visibility_scene_cameras(vis):
    """Three image sizes, three yaws, (nearly) one position."""
    assert [(c.image_width, c.image_height) for c in vis.cams] == [(64, 48), (80, 32), (48, 64)]
    pos = torch.stack([c.camera_center for c in vis.cams])
    assert float((pos - pos.mean(0)).norm(dim=1).max()) <= 0.11 and float(pos[:, 1:].abs().max()) < 1e-6
    fwd = torch.stack([c.world_view_transform[:3, 2] for c in vis.cams])  # the view direction, in world axes
    yaw = torch.rad2deg(torch.atan2(fwd[:, 0], fwd[:, 2]))
    assert torch.allclose(yaw, torch.tensor([30.0, 0.0, -5.0]), atol=1e-3) and float(fwd[:, 1].abs().max()) < 1e-6


def test_visibility_scene_patterns(vis, vis_prep):
    """Every Gaussian is seen by exactly the views its cluster was placed for, and each of the 8
    patterns over the three views holds at least 16 Gaussians."""
    seen = _seen(vis, vis_prep)
    for k, name in enumerate(NAMES):
        sel = vis.group == k
        assert np.array_equal(seen[sel], vis.pattern[sel]), (name, seen[sel].mean(0))
    code = seen @ np.array([1, 2, 4])
    counts = np.bincount(code, minlength=8)
    print("pattern counts (view0 + 2 view1 + 4 view2):", counts.tolist())
    assert (counts >= 16).all(), counts


def test_visibility_scene_has_every_cause_of_invisibility(vis, vis_prep):
    """A view may miss a Gaussian because its depth is at most 0.2, because its tile rectangle is empty
    (outside the frustum), or because its opacity is below 1/255: at least 16 Gaussians of each kind,
    the first two also among Gaussians that another view does see."""
    seen = _seen(vis, vis_prep)
    op = vis.leaves["opacities"].numpy().reshape(-1)
    tz = np.stack([q["tz"].numpy() for q in vis_prep], 1)
    rad = np.stack([q["radii"].numpy() for q in vis_prep], 1)
    near = tz <= 0.2
    frustum = (tz > 0.2) & (rad == 0)
    faint = (rad > 0) & (op[:, None] < 1.0 / 255.0)
    assert not (seen & (near | frustum | faint)).any()
    assert (~seen == (near | frustum | faint)).all()
    elsewhere = seen.any(1)
    print("near", int(near.any(1).sum()), "frustum", int(frustum.any(1).sum()), "faint", int(faint.any(1).sum()))
    assert (near.any(1) & elsewhere).sum() >= 16 and (near.all(1)).sum() >= 16
    assert (frustum.any(1) & elsewhere).sum() >= 16
    assert faint.all(1).sum() >= 16
    # the near ones that another view sees lie inside that missing view's frustum by direction: only the
    # depth test removes them there (view 1, whose half widths are tan = 0.91 and 0.364)
    k = NAMES.index("near_v0")
    ph = torch.cat([vis.leaves["means3D"].double(), torch.ones((seen.shape[0], 1), dtype=torch.float64)], 1)
    pv = (ph @ vis.cams[1].world_view_transform.double())[vis.group == k]
    assert (pv[:, 2] > 0).all() and ((pv[:, 0] / pv[:, 2]).abs() < math.tan(vis.cams[1].FoVx / 2)).all()
    # nothing sits at a decision: depths away from 0.2, opacities away from 1/255
    assert (np.abs(tz - 0.2) > 2e-3).all() and (np.abs(op - 1.0 / 255.0) > 5e-4).all()


@pytest.mark.parametrize("D", [1, 2, 3])
def test_visibility_scene_clamp_bits_differ_between_views(vis, vis_prep, D):
    """At least 16 Gaussians clamp a colour channel in one view and not in another, both seeing them;
    no colour lies within 0.05 of the clamp in the cluster built for it."""
    seen = _seen(vis, vis_prep)
    bits = np.stack([fvc.clamp_bits(vis.leaves, c, D) for c in vis.cams], 1)  # [P, view, channel]
    differ = np.zeros(seen.shape[0], bool)
    for a in range(3):
        for b in range(a + 1, 3):
            differ |= seen[:, a] & seen[:, b] & (bits[:, a] != bits[:, b]).any(1)
    print("Gaussians whose clamp bits differ between two views that see them:", int(differ.sum()))
    assert differ.sum() >= 16
    sel = vis.group == NAMES.index("clamp")
    m = vis.leaves["means3D"][sel].double()
    for v in (1, 2):
        d = torch.nn.functional.normalize(m - vis.cams[v].camera_center.double()[None], dim=1)
        c0 = dense_ref.sh_rgb(D, vis.leaves["shs"][sel].double(), d)[:, 0] + 0.5
        assert ((c0 > 0.05) if v == 1 else (c0 < -0.05)).all(), (v, c0)


def test_visibility_scene_few_pixels_near_a_threshold(vis):
    """At most the 2 % of the pixels that tests/test_gpu_dense.py tolerates are flagged as within 1e-5
    (relative) of an alpha / transmittance decision, in each view."""
    t = {k: v.double() for k, v in vis.leaves.items()}
    for v, c in enumerate(vis.cams):
        f = torch.float64
        _, radii, flag = dense_ref.render_local(
            t["means3D"], torch.zeros_like(t["means3D"]), t["opacities"], c.world_view_transform.to(f),
            c.full_proj_transform.to(f), c.camera_center.to(f), math.tan(c.FoVx / 2), math.tan(c.FoVy / 2),
            c.image_width, c.image_height, torch.zeros(3, dtype=f), shs=t["shs"], deg=3, scales=t["scales"],
            rots=t["rotations"])
        print(f"view {v}: flagged {int(flag.sum())}/{flag.numel()}, radii 1..{int(radii.max())}")
        assert float(flag.double().mean()) <= 0.02


@pytest.mark.parametrize("K", [1, 2, 8, 9, 16, 17])
def test_ring_cameras(K):
    cams = fvc.ring_cameras(K)
    assert len(cams) == K
    assert [(c.image_width, c.image_height) for c in cams] == [fvc.SIZES[v % 3] for v in range(K)]
    pos = torch.stack([c.camera_center for c in cams])
    assert torch.allclose(pos.norm(dim=1), torch.full((K,), 6.0), atol=1e-4)
    assert K == 1 or float((pos[0] - pos[1]).norm()) > 0.5  # distinct views


@pytest.mark.parametrize("K", [9, 17])
def test_marked_gaussians_are_seen_by_the_last_ring_camera_only(K):
    """layout_scene(marked=) with ring_cameras(last_target=): the marked Gaussians contribute to the
    last view and to no other; the last view is therefore the only one of its pass (views 8..K-1) that
    decides their gradient."""
    P, marked = 300, 24
    leaves = fvc.layout_scene(P, 3, 16, marked=marked)
    cams = fvc.ring_cameras(K, last_target=fvc.MARK_TARGET)
    op = leaves["opacities"].numpy()
    seen = np.stack([fvc.contributes(fvc.dense_prep(leaves, c, 3)["radii"].numpy(), op) for c in cams], 1)
    big = op.reshape(-1)[P - marked:] >= 1.0 / 255.0
    assert big.sum() >= 16
    assert seen[P - marked:, -1][big].all() and not seen[P - marked:, :-1].any()
    assert seen[:P - marked, :-1].mean() > 0.9  # the ball is in front of the other cameras


@pytest.mark.parametrize("D,M", fvc.LAYOUTS)
@pytest.mark.parametrize("kind", ["sh", "colors", "cov3d"])
def test_layout_scene(D, M, kind):
    P = 257
    leaves = fvc.layout_scene(P, D, M, kind)
    assert set(leaves) == {"means3D", "opacities", "colors" if kind == "colors" else "shs",
                           *(("cov3D",) if kind == "cov3d" else ("scales", "rotations"))}
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] == P for t in leaves.values())
    if kind != "colors":
        assert leaves["shs"].shape == (P, M, 3) and (leaves["shs"] != 0).all()
    # precomputed covariances are those of the scales and rotations of the same seed
    if kind == "cov3d":
        a = fvc.dense_prep(leaves, fvc.ring_cameras(3)[1], D)
        b = fvc.dense_prep(fvc.layout_scene(P, D, M, "sh"), fvc.ring_cameras(3)[1], D)
        assert torch.allclose(a["conic"], b["conic"], rtol=1e-4, atol=1e-6)
    seen = [float((fvc.dense_prep(leaves, c, D)["radii"] > 0).double().mean()) for c in fvc.ring_cameras(3)]
    assert min(seen) > 0.9, seen
