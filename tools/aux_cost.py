"""Cost of the aux outputs at C3 (1M Gaussians, SH3, 1920 x 1080): one process, run under `timeout`.

Two configurations of one view's forward + backward, 20 timed steps after 5 warm-up steps each:
  plain  GaussianRasterizer(...) -> (color, radii), backward of a colour loss
  aux    GaussianRasterizer(..., aux_outputs=True), backward with all three gradients present
Per configuration: the wall time of a step (synchronised, untimed kernels) and, in a second pass
with gs_profile_enable, the per-kernel HIP-event times of render_fwd / render_bwd / sum_records and
of the aux kernels.  The only way to get the two outputs without the feature is a second plain
render pass with colors_precomp = (1/z, 1, 0): twice the plain time, from the same file.
Writes profiles/aux_cost_c3.json (or --out)."""
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
# (the aux backward sums its records ten wide: sum_records_aux replaces sum_records there)
KERNELS = ("render_fwd", "render_bwd", "sum_records", "render_fwd_aux", "render_bwd_aux", "sum_records_aux",
           "depth_chain_aux", "preprocess_bwd")

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_cost_c3.json"))
a = ap.parse_args()

dev = torch.device("cuda:0")
lib = _native.load()
cam = gs_scenes.identity_camera(W, H)
sc = gs_scenes.random_gaussians(P, DEG, cam=cam, seed=0).to(dev)
params = [t.clone().requires_grad_(True) for t in (sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations)]
gC = gs_scenes.dl_dimage(H, W).to(dev)
gD = gs_scenes.dl_dimage(H, W, seed=2)[:1].contiguous().to(dev)
gA = gs_scenes.dl_dimage(H, W, seed=3)[:1].contiguous().to(dev)
rast = GaussianRasterizer(gs_scenes.raster_settings_for(cam, DEG, device=dev))


def step(aux):
    for p in params:
        p.grad = None
    m2 = torch.empty_like(params[0], requires_grad=True)
    out = rast(means3D=params[0], means2D=m2, opacities=params[2], shs=params[1], scales=params[3],
               rotations=params[4], aux_outputs=aux)
    if aux:
        torch.autograd.backward([out[0], out[2], out[3]], [gC, gD, gA])
    else:
        out[0].backward(gC)


def measure(aux):
    for _ in range(a.warmup):
        step(aux)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step(aux)
    torch.cuda.synchronize()
    wall_ms = 1e3 * (time.perf_counter() - t0) / a.steps
    lib.gs_profile_collect()
    lib.gs_profile_reset()
    lib.gs_profile_enable(1)
    for _ in range(a.steps):
        step(aux)
    torch.cuda.synchronize()
    stats = _native.profile_stats()
    lib.gs_profile_enable(0)
    lib.gs_profile_reset()
    kern = {k: round(1e3 * stats[k][0] / stats[k][1], 2) for k in KERNELS if k in stats}
    launches = {k: stats[k][1] // a.steps for k in KERNELS if k in stats}
    total = round(sum(1e3 * ms / a.steps for ms, _n in stats.values()), 1)
    return {"step_ms": round(wall_ms, 4), "kernel_us": kern, "launches_per_step": launches,
            "all_kernels_us_per_step": total}


plain, aux = measure(False), measure(True)
pk, ak = plain["kernel_us"], aux["kernel_us"]
res = {
    "workload": f"C3: {P} Gaussians SH{DEG} {W}x{H}", "steps": a.steps, "warmup": a.warmup,
    "device": torch.cuda.get_device_name(0), "plain": plain, "aux": aux,
    "aux_overhead_us": {
        "render_fwd": round(ak["render_fwd_aux"] - pk["render_fwd"], 2),
        "render_bwd": round(ak["render_bwd_aux"] - pk["render_bwd"], 2),
        "sum_records": round(ak["sum_records_aux"] - pk["sum_records"], 2),
        "depth_chain_aux": ak["depth_chain_aux"]},
    "step_overhead_ms": round(aux["step_ms"] - plain["step_ms"], 4),
    "second_plain_pass_ms": plain["step_ms"],
    "all_kernels_overhead_us": round(aux["all_kernels_us_per_step"] - plain["all_kernels_us_per_step"], 1),
    "second_plain_pass_kernels_us": plain["all_kernels_us_per_step"],
}
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
