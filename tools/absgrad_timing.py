"""render_bwd_abs + sum_records_abs + mean2d_absgrad against render_bwd + sum_records on one C3 view
(bench.py's scene): the library's launch profile (HIP events around each launch), one collect per
call, medians of 60 warm launches, the two backwards alternating in one process, in both numerics
modes.  `python tools/absgrad_timing.py [out.json]`; the committed record is
profiles/absgrad_timing_c3.json."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-skysphere_amd")]

import torch  # noqa: E402

import gs_scenes  # noqa: E402
from diff_gaussian_rasterization import _C, _native  # noqa: E402

N, WARM = 60, 5
dev = torch.device("cuda:0")
lib = _native.load()
P, deg, W, H = 1_000_000, 3, 1920, 1080
cam = gs_scenes.identity_camera(W, H)
sc = gs_scenes.random_gaussians(P, deg, cam=cam, seed=0).to(dev)
s = gs_scenes.raster_settings_for(cam, deg, device=dev)
e = torch.Tensor([])
dpix = gs_scenes.dl_dimage(H, W, seed=1, scale=1.0).to(dev)
WALK = {"plain": ("render_bwd", "sum_records"), "absgrad": ("render_bwd_abs", "sum_records_abs", "mean2d_absgrad")}
res = {}
for exact in (0, 1):
    lib.gs_set_exact_exp(exact)
    with torch.no_grad():
        R, color, radii, geom, binning, img = _C.rasterize_gaussians_two_call(
            s.bg, sc.means3D, e, sc.opacities, sc.scales, sc.rotations, s.scale_modifier, e, s.viewmatrix, s.projmatrix,
            s.tanfovx, s.tanfovy, H, W, sc.shs, deg, s.campos, False, False)

        def bwd(absgrad):
            return _C.backward_impl(s.bg, sc.means3D, radii, e, sc.scales, sc.rotations, s.scale_modifier, e,
                                    s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, dpix, sc.shs, deg, s.campos, geom,
                                    R, binning, img, False, want_all=True, **({"absgrad": True} if absgrad else {}))

        calls = {"plain": lambda: bwd(False), "absgrad": lambda: bwd(True)}
        per = {k: {} for k in calls}
        for it in range(WARM + N):
            for k, fn in calls.items():
                torch.cuda.synchronize()
                lib.gs_profile_collect()
                lib.gs_profile_reset()
                lib.gs_profile_enable(1)
                fn()
                torch.cuda.synchronize()
                st = _native.profile_stats()
                lib.gs_profile_enable(0)
                if it >= WARM:
                    for name, (ms, n) in st.items():
                        per[k].setdefault(name, []).append(1e3 * ms / max(n, 1))
        lib.gs_profile_reset()
    out = {k: {name: round(statistics.median(v), 2) for name, v in d.items()} for k, d in per.items()}
    for k, names in WALK.items():
        out[k]["walk_and_sums"] = round(sum(out[k][n] for n in names), 2)
    out["ratio"] = round(out["absgrad"]["walk_and_sums"] / out["plain"]["walk_and_sums"], 4)
    out["instances"] = int(R)
    res["exact" if exact else "fast"] = out
    print("exact" if exact else "fast", json.dumps(out))
lib.gs_set_exact_exp(0)
res["note"] = ("median us per launch over %d warm launches (HIP events of the library's launch profile), C3 view: "
               "1M Gaussians SH3 1920x1080, identity camera, seed 0; walk_and_sums = render_bwd + sum_records "
               "(absgrad: render_bwd_abs + sum_records_abs + mean2d_absgrad), ratio = absgrad / plain" % N)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
