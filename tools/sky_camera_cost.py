"""Cost of the skysphere's view-matrix gradient: a 1920 x 1080 image with a 1024 x 2048 texture, one
process, run under `timeout`.

Three configurations of gs_sky.compose + backward, 20 timed steps after 5 warm-up steps each:
  plain       dL/dalpha and dL/dtexture (k_sky_bwd<false>), the view matrix a constant
  with_view   camera_grads=True, the view matrix requires grad as well (k_sky_bwd<true> + k_sky_cam_finish)
  view_alone  camera_grads=True, alpha and texture frozen: no texture scratch, no scatter
Per configuration: the wall time of a step (synchronised, untimed kernels) and, in a second pass with
gs_profile_enable, the per-kernel HIP-event times.  The camera is a look-at pose (not the identity).
Writes profiles/sky_camera_cost.json (or --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gaussian-splatting-skysphere_amd"), ROOT]

import torch  # noqa: E402

import gs_scenes  # noqa: E402
import gs_sky  # noqa: E402
from diff_gaussian_rasterization import _native  # noqa: E402

W, H, HS, WS = 1920, 1080, 1024, 2048

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sky_camera_cost.json"))
a = ap.parse_args()

dev = torch.device("cuda:0")
lib = _native.load()
cam = gs_scenes.look_at_camera((0.7, -0.4, -1.1), (0.1, 0.2, 4.0), W, H)
base = gs_scenes.raster_settings_for(cam, 0, device=dev)
gen = torch.Generator().manual_seed(7)
color = torch.rand((3, H, W), generator=gen).to(dev)
alpha0 = torch.rand((H, W), generator=gen).to(dev)
tex0 = torch.rand((3, HS, WS), generator=gen).to(dev)
g = torch.randn((3, H, W), generator=gen).to(dev)
# (camera_grads, alpha and texture require grad)
CONFIGS = {"plain": (False, True), "with_view": (True, True), "view_alone": (True, False)}


def measure(name):
    flag, others = CONFIGS[name]
    alpha, tex = alpha0.clone().requires_grad_(others), tex0.clone().requires_grad_(others)
    V = base.viewmatrix.detach().clone().requires_grad_(flag)
    s = base._replace(viewmatrix=V)

    def step():
        alpha.grad = tex.grad = V.grad = None
        gs_sky.compose(color, alpha, tex, s, camera_grads=flag).backward(g)

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
    kern = {k: round(1e3 * ms / n, 2) for k, (ms, n) in stats.items()}
    return {"step_ms": round(wall_ms, 4), "kernel_us": kern,
            "launches_per_step": {k: n // a.steps for k, (_ms, n) in stats.items()},
            "backward_kernels_us": round(sum(v for k, v in kern.items() if k != "sky_fwd"), 2)}


res = {"workload": f"sky compose + backward, {W}x{H}, texture {HS}x{WS}, look-at camera", "steps": a.steps,
       "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "library": os.path.relpath(_native.LIB_PATH, ROOT)}
for name in CONFIGS:
    res[name] = measure(name)
res["view_overhead"] = {
    "sky_bwd_cam_minus_sky_bwd_us": round(res["with_view"]["kernel_us"]["sky_bwd_cam"] - res["plain"]["kernel_us"]["sky_bwd"], 2),
    "sky_cam_finish_us": res["with_view"]["kernel_us"]["sky_cam_finish"],
    "backward_kernels_us": round(res["with_view"]["backward_kernels_us"] - res["plain"]["backward_kernels_us"], 2),
    "step_ms": round(res["with_view"]["step_ms"] - res["plain"]["step_ms"], 4)}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
