"""gs_pose.CameraTwist on the CPU: the chain from a twist to the three camera tensors."""
import pytest
import torch

import gs_scenes

CAMS = {
    "look_at": lambda: gs_scenes.look_at_camera((0.7, -0.4, -1.1), (0.1, 0.2, 4.0), 96, 64),
    "identity": lambda: gs_scenes.identity_camera(40, 30),
    "wide": lambda: gs_scenes.look_at_camera((0.3, 0.2, -1.0), (0.1, -5.0, 0.2), 72, 40, fovy_deg=100.0),
}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("name", list(CAMS))
def test_zero_twist_is_the_camera(name):
    import gs_pose

    cam = CAMS[name]()
    twist = gs_pose.CameraTwist(cam)
    assert [n for n, _ in twist.named_parameters()] == ["delta"]
    assert twist.delta.shape == (6,) and not twist.delta.any() and twist.delta.dtype == torch.float32
    base = gs_scenes.raster_settings_for(cam, 0, device="cpu")
    s = twist.settings(base)
    for t in (s.viewmatrix, s.projmatrix, s.campos):
        assert t.requires_grad and not t.is_leaf and t.dtype == torch.float32
    assert s.viewmatrix.shape == (4, 4) and s.projmatrix.shape == (4, 4) and s.campos.shape == (3,)
    assert torch.equal(_bits(s.viewmatrix), _bits(cam.world_view_transform))
    for got, want in ((s.projmatrix, cam.full_proj_transform), (s.campos, cam.camera_center)):
        assert float((got.detach() - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max())
    # everything else of the settings is kept
    for k in ("image_height", "image_width", "tanfovx", "tanfovy", "sh_degree", "scale_modifier"):
        assert getattr(s, k) == getattr(base, k)
    assert s.bg is base.bg


def test_gradcheck_fp64():
    import gs_pose

    twist = gs_pose.CameraTwist(CAMS["look_at"]()).double()
    assert twist.delta.dtype == torch.float64 and twist.view0.dtype == torch.float64

    def f(delta):
        twist.delta.data = delta.data  # the module's chain, evaluated at delta
        view = twist.view0 @ gs_pose.twist_matrix(delta)
        return view, view @ twist.projection, view.inverse()[3, :3]

    for d in (torch.zeros(6, dtype=torch.float64),
              torch.tensor([0.02, -0.03, 0.015, 0.1, -0.2, 0.05], dtype=torch.float64)):
        d = d.clone().requires_grad_(True)
        assert torch.autograd.gradcheck(f, (d,), eps=1e-6, atol=1e-7)
        with torch.no_grad():
            twist.delta.copy_(d)
        for got, want in zip(twist.camera_tensors(), f(d)):
            assert torch.equal(got, want)


def test_a_pure_rotation_leaves_the_translation_row():
    import gs_pose

    cam = CAMS["look_at"]()
    twist = gs_pose.CameraTwist(cam).double()
    with torch.no_grad():
        twist.delta.copy_(torch.tensor([0.2, -0.1, 0.3, 0.0, 0.0, 0.0]))
    view, _, campos = (t.detach() for t in twist.camera_tensors())
    # exp(delta^) of a pure rotation has the last row (0, 0, 0, 1): the camera turns about its own centre.
    # In view = view0 exp(delta^) that leaves column 3 and the camera centre alone; the translation row
    # is T R, untouched as a row only for a camera at the origin (T = 0, below).
    E = gs_pose.twist_matrix(twist.delta.detach())
    assert torch.equal(E[3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64))
    assert torch.equal(E[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64))
    assert torch.equal(view[:, 3], twist.view0[:, 3])
    assert float((campos - twist.view0.inverse()[3, :3]).abs().max()) < 1e-14
    assert float((view[3, :3].norm() - twist.view0[3, :3].norm()).abs()) < 1e-14
    R = E[:3, :3]
    assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-14
    assert float((view[:3, :3] - twist.view0[:3, :3]).abs().max()) > 0.05
    origin = gs_pose.CameraTwist(gs_scenes.look_at_camera((0, 0, 0), (0.3, -0.4, -3.0), 96, 64)).double()
    with torch.no_grad():
        origin.delta.copy_(twist.delta)
    assert torch.equal(origin.camera_tensors()[0][3], origin.view0[3])
    # a translation moves the last row only, by v
    with torch.no_grad():
        twist.delta.copy_(torch.tensor([0.0, 0.0, 0.0, 0.5, -0.25, 0.125]))
    moved = twist.camera_tensors()[0].detach()
    assert torch.equal(moved[:3], twist.view0[:3])
    assert float((moved[3, :3] - twist.view0[3, :3] - twist.delta.detach()[3:]).abs().max()) < 1e-15


def test_backward_reaches_delta():
    import gs_pose

    twist = gs_pose.CameraTwist(CAMS["wide"]())
    s = twist.settings(gs_scenes.raster_settings_for(CAMS["wide"](), 0, device="cpu"))
    (s.viewmatrix.sum() + s.projmatrix.sum() + s.campos.sum()).backward()
    assert twist.delta.grad is not None and twist.delta.grad.shape == (6,) and bool(twist.delta.grad.abs().min() > 0)
