"""Scenes, raw-parameter edges and optimizer states for the fused per-Gaussian backward + Adam step
(k_preprocess_bwd_adam, train_step(fuse_adam=True); test infrastructure, pure torch / numpy).

The other fused-Adam tests fill one camera's frustum with random Gaussians, step every group with the same
hyper-parameters and start from zero moments.  Here

  model_scene(P)    the first P rows of fused_views_cases.visibility_scene() in a fixed random order: three
                    cameras of different image sizes, and from a few rows on Gaussians that a camera does
                    not see (behind it, outside its frustum, too faint) next to ones it sees
  poke_raw(model)   raw-parameter edges of the activations on Gaussians that every camera sees: a zero and
                    a 1e-8-scaled quaternion, saturated opacities, a vanishing scale
  P_EDGES           row counts whose last workgroup holds 1, 2, 3, 4, 255, 256, 1, 2, 3 and 96 rows
  odd_hyper(opt)    a distinct weight decay and step count per group, seeded non-zero moments
  ref_forward()     one view by the fp64 dense reference (tests/dense_ref.py) behind torch's own cat / sigmoid /
                    exp / normalize of the raw parameters: autograd then gives their gradients
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import fused_views_cases as fvc
import gs_scenes

P_EDGES = (1, 2, 3, 4, 255, 256, 257, 258, 259, 352)
NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
# the first four rows come from the clusters all, v0, v1v2, v0v1, and the last row of every size in P_EDGES -- the
# row whose floats are the scalar tail of features_dc / features_rest -- is seen by some camera (from 255 on by
# camera 0), so the tail gets a gradient (tests/test_fused_adam_cases.py)
PERM_SEED = 1385
SEEN_BY_ALL = ("all", "clamp")

# odd_hyper: per group (xyz, f_dc, f_rest, opacity, scaling, rotation)
WEIGHT_DECAYS = (0.01, 0.02, 0.03, 0.05, 0.07, 0.11)
STEPS = (1, 2, 5, 9, 17, 33)
ODD_BETAS, ODD_EPS = (0.8, 0.99), 1e-8

# The tests' image gradient: N(2, 1) per pixel and channel, one seed per camera.  Each cluster of the
# scene stacks its 32 Gaussians on a few pixels, and most directions have y ~ 0, so many SH coefficients get
# a gradient of 1e-3 .. 1e-5 of the tensor's largest.  With a zero-mean dL/dpix the largest is a lucky sum
# and 6 to 9 % of features_rest lie inside the fp64 comparison's own error bound under every seed tried
# (600 per camera); the mean of 2 makes the sums add up and leaves at most 4 % there.
# tests/test_fused_adam_cases.py asserts the 5 % cap from the reference alone.
DPIX_SEEDS, DPIX_MEAN, DPIX_SCALE = (101, 102, 103), 2.0, 1.0
# (frac of max|ref| in the bound 1e-5 |ref| + frac max|ref|: tests/test_gpu_dense.py's, the covariance chain 5e-5)
BOUND_FRAC = {"_xyz": 5e-5, "_features_dc": 1e-5, "_features_rest": 1e-5, "_opacity": 1e-5, "_scaling": 5e-5,
              "_rotation": 5e-5}
RTOL = 1e-5


@functools.lru_cache(maxsize=None)
def _vis():
    return fvc.visibility_scene()


@functools.lru_cache(maxsize=None)
def _perm():
    n = _vis().leaves["means3D"].shape[0]
    return torch.randperm(n, generator=torch.Generator().manual_seed(PERM_SEED))


def model_rows(P):
    """[P] int64: the row of visibility_scene() that row i of model_scene(P) is (a copy of)."""
    perm = _perm()
    return perm[torch.arange(P) % perm.shape[0]]


def model_groups(P):
    """[P] names of the cluster (fused_views_cases.VIS_GROUPS) each row of model_scene(P) comes from."""
    names = [g[0] for g in fvc.VIS_GROUPS]
    return [names[k] for k in _vis().group[model_rows(P).numpy()]]


def model_scene(P, jitter_seed=17):
    """(gs_scenes.GaussianScene of P Gaussians with 16 SH coefficients, the three cameras).  Rows past the
    scene's 352 repeat it with a small jitter of the means (1e-3 of the distance) and the colours."""
    vis = _vis()
    rows = model_rows(P)
    t = {k: v[rows].clone() for k, v in vis.leaves.items()}
    n = _perm().shape[0]
    if P > n:
        g = torch.Generator().manual_seed(jitter_seed)
        t["means3D"][n:] *= 1.0 + 1e-3 * (2.0 * torch.rand((P - n, 1), generator=g) - 1.0)
        t["shs"][n:, 0] += 0.01 * torch.randn((P - n, 3), generator=g)
    sc = gs_scenes.GaussianScene(t["means3D"].contiguous(), t["opacities"].contiguous(), t["scales"].contiguous(),
                                 t["rotations"].contiguous(), t["shs"].contiguous(), 3)
    return sc, list(vis.cams)


# what poke_raw writes, in the order in which the rows seen by every camera are handed out (a scene with
# fewer such rows gets the first ones only)
POKES = (("_rotation", "zero"), ("_rotation", 1e-8), ("_opacity", 15.0), ("_scaling", -20.0), ("_opacity", -15.0))


def poke_rows(P):
    """The rows poke_raw touches in a model of model_scene(P): one per entry of POKES, in that order."""
    groups = model_groups(min(P, _perm().shape[0]))
    return [i for i, g in enumerate(groups) if g in SEEN_BY_ALL][:len(POKES)]


def poke_raw(model):
    """Overwrites, under no_grad, raw rows of Gaussians that all three cameras see: one _rotation row with
    zeros (F.normalize's 1e-12 clamp), one scaled by 1e-8, one _opacity row with +15 and one with -15
    (sigmoid saturated; the latter falls below 1/255 and is no longer rendered), one _scaling row with
    -20.  Returns {(parameter name, what): row}."""
    done = {}
    with torch.no_grad():
        for (name, what), i in zip(POKES, poke_rows(model.P)):
            p = getattr(model, name)
            if what == "zero":
                p[i] = 0.0
            elif name == "_rotation":
                p[i] *= what
            else:
                p[i] = what
            done[(name, what)] = i
    return done


def odd_hyper(optimizer, betas=ODD_BETAS, eps=ODD_EPS, maximize=False, seed=23):
    """On each of the optimizer's six groups: its own non-zero weight_decay (WEIGHT_DECAYS) and its own
    step count so far (STEPS), with seeded moments -- exp_avg ~ 0.1 N(0, 1), exp_avg_sq ~ 0.01 U(0, 1) --
    drawn on the host so that two optimizers given the same seed hold the same floats; betas, eps and
    maximize shared by the groups."""
    g = torch.Generator().manual_seed(seed)
    assert len(optimizer.param_groups) == 6
    for k, group in enumerate(optimizer.param_groups):
        group["weight_decay"], group["betas"], group["eps"], group["maximize"] = WEIGHT_DECAYS[k], betas, eps, maximize
        p, = group["params"]
        optimizer.state[p] = {
            "step": torch.tensor(float(STEPS[k]), dtype=torch.float32),
            "exp_avg": (0.1 * torch.randn(p.shape, generator=g)).to(p.device),
            "exp_avg_sq": (0.01 * torch.rand(p.shape, generator=g)).to(p.device),
        }


def seen(radii, opacities):
    """[P] bool (numpy): fused_views_cases.contributes -- the Gaussians that get tile instances."""
    return fvc.contributes(np.asarray(radii), np.asarray(opacities))


def dpix_for(cam_index, cam):
    """dL/dimage [3, H, W] (float32, host) of camera `cam_index`."""
    return DPIX_MEAN + gs_scenes.dl_dimage(cam.image_height, cam.image_width, seed=DPIX_SEEDS[cam_index],
                                           scale=DPIX_SCALE)


def raw_of_scene(sc):
    """TrainModel's raw parameters of an activated scene (gs_train_step.TrainModel.__init__), float32 on
    the scene's device, in the order of NAMES."""
    op = sc.opacities.clamp(1e-6, 1 - 1e-6)
    return [sc.means3D.clone(), sc.shs[:, :1].clone().contiguous(), sc.shs[:, 1:].clone().contiguous(),
            torch.log(op / (1 - op)), torch.log(sc.scales), sc.rotations.clone()]


def ref_forward(raw, cam, deg, device="cpu"):
    """The fp64 dense reference of one view from the six raw parameters (any float dtype; taken to
    float64): the activations in torch (cat, sigmoid, exp, F.normalize), then dense_ref.render_local.
    Returns (leaves: the six float64 raw tensors that require grad, image, radii, flag)."""
    import dense_ref

    f = torch.float64
    leaves = [t.detach().to(device, f).clone().requires_grad_(True) for t in raw]
    xyz, dc, rest, op, sc, rot = leaves
    W, H = cam.image_width, cam.image_height
    img, radii, flag = dense_ref.render_local(
        xyz, torch.zeros_like(xyz), torch.sigmoid(op), cam.world_view_transform.to(device, f),
        cam.full_proj_transform.to(device, f), cam.camera_center.to(device, f), math.tan(cam.FoVx / 2),
        math.tan(cam.FoVy / 2), W, H, torch.zeros(3, dtype=f, device=device), shs=torch.cat((dc, rest), dim=1),
        deg=deg, scales=torch.exp(sc), rots=torch.nn.functional.normalize(rot))
    return leaves, img, radii, flag


def ref_rects(raw, cam, deg, device="cpu"):
    """[P, 4] int64 tile rectangles (x0, y0, x1, y1) of the fp64 reference, numpy."""
    f = torch.float64
    xyz, dc, rest, op, sc, rot = (t.detach().to(device, f) for t in raw)
    leaves = dict(means3D=xyz, opacities=torch.sigmoid(op), shs=torch.cat((dc, rest), dim=1), scales=torch.exp(sc),
                  rotations=torch.nn.functional.normalize(rot))
    q = fvc.dense_prep(leaves, cam.to(device) if device != "cpu" else cam, deg)
    return torch.stack([q["x0"], q["y0"], q["x1"], q["y1"]], 1).to(torch.int64).cpu().numpy()


def widen_flags(flag, rects, rdiff):
    """tests/test_gpu_dense.py: a Gaussian whose fp32 radius differs composites into a rectangle up to one
    tile wider; its pixels are flagged too.  flag [H, W] bool numpy (changed in place and returned)."""
    for i in np.nonzero(rdiff)[0]:
        x0, y0, x1, y1 = rects[i]
        flag[max(16 * y0 - 16, 0):16 * y1 + 16, max(16 * x0 - 16, 0):16 * x1 + 16] = True
    return flag


def bound(name, ref):
    """The element-wise error bound of a float64 numpy gradient tensor `ref` (its kept rows):
    1e-5 |ref| + frac max|ref| (BOUND_FRAC)."""
    return RTOL * np.abs(ref) + BOUND_FRAC[name] * float(np.abs(ref).max(initial=0.0))


def active_columns(name, deg):
    """features_rest's coefficients of the active degree (the others have no gradient); None: all."""
    return (deg + 1) ** 2 - 1 if name == "_features_rest" else None


def inside_share(name, ref, visible, deg):
    """(share, exact zeros, count): among the elements of the visible rows (the active columns of
    features_rest) the share whose |ref| is positive and within its own bound -- the sign of the first
    Adam step is not decided by the reference there -- and the number of elements whose reference gradient
    is exactly zero (a colour channel clamped at 0 has none: those are held to an exact check instead)."""
    r = ref[visible]
    k = active_columns(name, deg)
    b = bound(name, ref)[visible]
    if k is not None:
        r, b = r[:, :k], b[:, :k]
    inside = (np.abs(r) <= b) & (r != 0)
    return float(inside.mean()) if r.size else 0.0, int((r == 0).sum()), int(r.size)
