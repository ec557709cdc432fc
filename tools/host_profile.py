"""Host-side cost of the eager rasterizer call at a small workload (C2 by default): cProfile of
N forward + backward iterations through GaussianRasterizer, sorted by own time.  The GPU work of
such a step is shorter than its Python / ctypes / allocator work, so this is where an eager C1 / C2
iteration goes.  --aux / --camera: the aux_outputs=True / camera_grads=True calls (loss over every
output; the three camera tensors require grad)."""
import argparse
import cProfile
import os
import pstats
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# GS_PKG: another copy of the package (an A/B of host-side changes in one call)
sys.path[:0] = [os.environ.get("GS_PKG", os.path.join(ROOT, "gaussian-splatting-skysphere_amd")), ROOT]

import torch  # noqa: E402

import gs_scenes  # noqa: E402
from diff_gaussian_rasterization import GaussianRasterizer  # noqa: E402

WL = {"c1": (10_000, 0, 256, 256), "c2": (100_000, 3, 800, 800)}
ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="c2", choices=sorted(WL))
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--capacity", type=int, default=None,
                help="bounded forwards (binning_capacity): no instance-count host wait per forward")
ap.add_argument("--no-profile", action="store_true")
ap.add_argument("--aux", action="store_true", help="aux_outputs=True")
ap.add_argument("--camera", action="store_true", help="camera_grads=True")
a = ap.parse_args()
P, deg, W, H = WL[a.workload]
dev = torch.device("cuda:0")
cam = gs_scenes.identity_camera(W, H)
sc = gs_scenes.random_gaussians(P, deg, cam=cam, seed=0).to(dev)
params = [t.clone().requires_grad_(True) for t in (sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations)]
dpix = gs_scenes.dl_dimage(H, W).to(dev)
settings = gs_scenes.raster_settings_for(cam, deg, device=dev)
cams = []
if a.camera:
    cams = [t.detach().clone().contiguous().requires_grad_(True)
            for t in (settings.viewmatrix, settings.projmatrix, settings.campos)]
    settings = settings._replace(viewmatrix=cams[0], projmatrix=cams[1], campos=cams[2])
r = GaussianRasterizer(settings)
daux = [dpix[:1].contiguous(), dpix[1:2].contiguous()]


def step():
    for p in params + cams:
        p.grad = None
    m2 = torch.zeros_like(params[0], requires_grad=True)
    out = r(means3D=params[0], means2D=m2, opacities=params[2], shs=params[1], scales=params[3], rotations=params[4],
            binning_capacity=a.capacity, aux_outputs=a.aux, camera_grads=a.camera)
    if a.aux:
        torch.autograd.backward([out[0], out[2], out[3]], [dpix] + daux)
    else:
        out[0].backward(dpix)


for _ in range(20):
    step()
torch.cuda.synchronize()
t = time.perf_counter()
for _ in range(a.steps):
    step()
torch.cuda.synchronize()
print(os.environ.get("GS_PKG", "(this tree)"))
print(f"{a.workload} eager{' aux' if a.aux else ''}{' camera' if a.camera else ''}"
      f"{'' if a.capacity is None else f' bounded({a.capacity})'}: "
      f"{1e3 * (time.perf_counter() - t) / a.steps:.4f} ms / iteration")
if a.capacity is not None:
    import diff_gaussian_rasterization as dgr  # noqa: E402
    dgr.bounded_status()
# host time alone: each iteration after the device has drained (no overlap with kernels)
tot = 0.0
for _ in range(a.steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    step()
    tot += time.perf_counter() - t
torch.cuda.synchronize()
print(f"  launch-side time per iteration from an idle device: {1e3 * tot / a.steps:.4f} ms")
if a.no_profile:
    sys.exit(0)
pr = cProfile.Profile()
pr.enable()
for _ in range(a.steps):
    step()
torch.cuda.synchronize()
pr.disable()
pstats.Stats(pr).sort_stats("tottime").print_stats(25)
