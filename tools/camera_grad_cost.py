"""Cost of camera_grads=True at C3 (1M Gaussians, SH3, 1920 x 1080): one process, run under `timeout`.

Three configurations of one view's forward + backward, 20 timed steps after 5 warm-up steps each:
  plain     GaussianRasterizer(...) with constant camera tensors
  view      camera_grads=True, only viewmatrix requires grad (k_camera_grad<-1>: no SH row read)
  all       camera_grads=True, viewmatrix, projmatrix and campos require grad (k_camera_grad<3>)
Per configuration: the wall time of a step (synchronised, untimed kernels) and, in a second pass with
gs_profile_enable, the per-kernel HIP-event times of the record sums, the per-Gaussian backward and
the two camera kernels.  The camera is a look-at pose (not the identity).  GSRAST_LIB selects the
library build (the reduction A/B: make BUILD=build_bfly EXTRA=-DGS_CAMGRAD_BUTTERFLY).
Writes profiles/camera_grad_cost_c3.json (or --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gaussian-splatting-skysphere_amd"), ROOT]

import torch  # noqa: E402

import gs_scenes  # noqa: E402
from diff_gaussian_rasterization import GaussianRasterizer, _native  # noqa: E402

P, DEG, W, H = 1_000_000, 3, 1920, 1080
KERNELS = ("render_bwd", "sum_records", "preprocess_bwd", "camera_grad", "camera_grad_finish")

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_grad_cost_c3.json"))
a = ap.parse_args()

dev = torch.device("cuda:0")
lib = _native.load()
cam = gs_scenes.look_at_camera((0.7, -0.4, -1.1), (0.1, 0.2, 4.0), W, H)
sc = gs_scenes.random_gaussians(P, DEG, cam=cam, seed=0).to(dev)
params = [t.clone().requires_grad_(True) for t in (sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations)]
gC = gs_scenes.dl_dimage(H, W).to(dev)
base = gs_scenes.raster_settings_for(cam, DEG, device=dev)
CONFIGS = {"plain": (False, (False, False, False)), "view": (True, (True, False, False)),
           "all": (True, (True, True, True))}


def rasterizer(req):
    cams = [t.detach().clone().contiguous().requires_grad_(r)
            for t, r in zip((base.viewmatrix, base.projmatrix, base.campos), req)]
    return GaussianRasterizer(base._replace(viewmatrix=cams[0], projmatrix=cams[1], campos=cams[2])), cams


def measure(name):
    on, req = CONFIGS[name]
    rast, cams = rasterizer(req)

    def step():
        for p in params + cams:
            p.grad = None
        m2 = torch.empty_like(params[0], requires_grad=True)
        out = rast(means3D=params[0], means2D=m2, opacities=params[2], shs=params[1], scales=params[3],
                   rotations=params[4], camera_grads=on)
        out[0].backward(gC)

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    wall_ms = 1e3 * (time.perf_counter() - t0) / a.steps
    lib.gs_profile_collect()
    lib.gs_profile_reset()
    lib.gs_profile_enable(1)
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    stats = _native.profile_stats()
    lib.gs_profile_enable(0)
    lib.gs_profile_reset()
    kern = {k: round(1e3 * stats[k][0] / stats[k][1], 2) for k in KERNELS if k in stats}
    launches = {k: stats[k][1] // a.steps for k in KERNELS if k in stats}
    total = round(sum(1e3 * ms / a.steps for ms, _n in stats.values()), 1)
    return {"step_ms": round(wall_ms, 4), "kernel_us": kern, "launches_per_step": launches,
            "all_kernels_us_per_step": total}


res = {"workload": f"C3: {P} Gaussians SH{DEG} {W}x{H}, look-at camera", "steps": a.steps, "warmup": a.warmup,
       "device": torch.cuda.get_device_name(0), "library": os.path.relpath(_native.LIB_PATH, ROOT)}
for name in CONFIGS:
    res[name] = measure(name)
for name in ("view", "all"):
    k = res[name]["kernel_us"]
    res[name + "_overhead"] = {
        "camera_kernels_us": round(k["camera_grad"] + k["camera_grad_finish"], 2),
        "step_ms": round(res[name]["step_ms"] - res["plain"]["step_ms"], 4),
        "all_kernels_us": round(res[name]["all_kernels_us_per_step"] - res["plain"]["all_kernels_us_per_step"], 1)}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
