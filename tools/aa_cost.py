"""Cost of antialiasing=True at C3 (1M Gaussians, SH3, 1920 x 1080): one process, run under `timeout`.

Two configurations of one view's forward + backward, 20 timed steps after 5 warm-up steps each:
  plain  GaussianRasterizer(...)                       k_preprocess<3>, k_preprocess_bwd_stage<false>
  aa     GaussianRasterizer(...)(antialiasing=True)    k_preprocess_aa<3>, k_preprocess_bwd_reg_aa<3>
Per configuration the per-kernel HIP-event times (gs_profile_enable) of the two kernels the switch
changes, the two renders (the antialiased opacities shrink the splats' alpha >= 1/255 ellipses, so
there are fewer instances) and the sum over all kernels.  GSRAST_NO_EXT=1 is set so that both
configurations take the same two-call host path.  Writes profiles/aa_cost_c3.json (or --out)."""
import argparse
import json
import os
import sys

os.environ["GSRAST_NO_EXT"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gaussian-splatting-skysphere_amd"), ROOT]

import torch  # noqa: E402

import gs_scenes  # noqa: E402
from diff_gaussian_rasterization import GaussianRasterizer, _native, last_num_rendered  # noqa: E402

P, DEG, W, H = 1_000_000, 3, 1920, 1080
KERNELS = ("preprocess", "preprocess_bwd", "render_fwd", "render_bwd", "sum_records")

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aa_cost_c3.json"))
a = ap.parse_args()

dev = torch.device("cuda:0")
lib = _native.load()
cam = gs_scenes.identity_camera(W, H)
sc = gs_scenes.random_gaussians(P, DEG, cam=cam, seed=0).to(dev)
params = [t.clone().requires_grad_(True) for t in (sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations)]
gC = gs_scenes.dl_dimage(H, W).to(dev)
rast = GaussianRasterizer(gs_scenes.raster_settings_for(cam, DEG, device=dev))


def measure(aa):
    def step():
        for p in params:
            p.grad = None
        m2 = torch.empty_like(params[0], requires_grad=True)
        out = rast(means3D=params[0], means2D=m2, opacities=params[2], shs=params[1], scales=params[3],
                   rotations=params[4], antialiasing=aa)
        out[0].backward(gC)

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    lib.gs_profile_collect()
    lib.gs_profile_reset()
    lib.gs_profile_enable(1)
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    stats = _native.profile_stats()
    lib.gs_profile_enable(0)
    lib.gs_profile_reset()
    return {"kernel_us": {k: round(1e3 * stats[k][0] / stats[k][1], 2) for k in KERNELS if k in stats},
            "all_kernels_us_per_step": round(sum(1e3 * ms / a.steps for ms, _n in stats.values()), 1),
            "instances": last_num_rendered()}


res = {"workload": f"C3: {P} Gaussians SH{DEG} {W}x{H}", "steps": a.steps, "warmup": a.warmup,
       "device": torch.cuda.get_device_name(0), "plain": measure(False), "aa": measure(True)}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
