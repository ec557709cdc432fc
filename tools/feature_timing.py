"""feature_fwd and feature_bwd_walk + feature_sum at C = 3, G and 4 G against render_fwd and
render_bwd + sum_records of the same C3 view (bench.py's scene): the library's launch profile (HIP
events around each launch), one collect per call, medians of 30 warm calls, the paths alternating, in
both numerics modes.  Per call and kernel name: the summed time of its launches in us and their
number (the backward runs one walk and one reduce per channel group; the forward one launch with the
groups on grid.y).  `python tools/feature_timing.py [out.json]`; the committed record is
profiles/feature_timing_c3.json."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-skysphere_amd")]

import torch  # noqa: E402

import gs_scenes  # noqa: E402
from diff_gaussian_rasterization import _C, _native  # noqa: E402

N, WARM = 30, 3
dev = torch.device("cuda:0")
lib = _native.load()
P, deg, W, H = 1_000_000, 3, 1920, 1080
G = _C.feature_group_channels()
cam = gs_scenes.identity_camera(W, H)
sc = gs_scenes.random_gaussians(P, deg, cam=cam, seed=0).to(dev)
s = gs_scenes.raster_settings_for(cam, deg, device=dev)
e = torch.Tensor([])
gen = torch.Generator().manual_seed(1)
dpix = torch.randn((3, H, W), generator=gen).to(dev)
Cs = (3, G, 4 * G)
feats = {C: torch.randn((P, C), generator=gen).to(dev) for C in Cs}
grads = {C: torch.randn((C, H, W), generator=gen).to(dev) for C in Cs}
outs = {C: torch.empty((C, H, W), device=dev) for C in Cs}
res = {}
for exact in (0, 1):
    lib.gs_set_exact_exp(exact)
    with torch.no_grad():

        def fwd():
            return _C.rasterize_gaussians_two_call(
                s.bg, sc.means3D, e, sc.opacities, sc.scales, sc.rotations, s.scale_modifier, e, s.viewmatrix,
                s.projmatrix, s.tanfovx, s.tanfovy, H, W, sc.shs, deg, s.campos, False, False)

        R, color, radii, geom, binning, img = fwd()
        args = (R, radii, geom, binning, img, s.viewmatrix, s.projmatrix, s.campos, s.tanfovx, s.tanfovy, H, W)

        def bwd():
            return _C.backward_render(s.bg, s.viewmatrix, s.projmatrix, s.campos, s.tanfovx, s.tanfovy, dpix, P, deg,
                                      16, geom, R, binning, img, False, False)

        calls = {"stats": lambda: _C.contribution_stats(*args), "bwd": bwd}
        for C in Cs:
            calls[f"feature_fwd_C{C}"] = lambda C=C: _C.feature_forward(*args, feats[C], out=outs[C])
            calls[f"feature_bwd_C{C}"] = lambda C=C: _C.feature_backward(*args, grads[C])
        calls["fwd"] = fwd  # last: it rewrites the view's buffers with the same words
        per = {k: {} for k in calls}
        for it in range(WARM + N):
            for k, fn in calls.items():
                torch.cuda.synchronize()
                lib.gs_profile_collect()
                lib.gs_profile_reset()
                lib.gs_profile_enable(1)
                keep = fn()
                torch.cuda.synchronize()
                st = _native.profile_stats()
                lib.gs_profile_enable(0)
                if k == "fwd":  # the buffers the other calls hold
                    R, color, radii, geom, binning, img = keep
                    args = (R, radii, geom, binning, img) + args[5:]
                if it >= WARM:
                    for name, (ms, n) in st.items():
                        per[k].setdefault(name, []).append((1e3 * ms, n))
        lib.gs_profile_reset()
    out = {}
    for k, d in per.items():
        names = ("render_fwd",) if k == "fwd" else tuple(d)
        out[k] = {name: {"us": round(statistics.median(v[0] for v in d[name]), 2), "launches": d[name][0][1]}
                  for name in names if name in d}
    out["instances"] = int(R)
    res["exact" if exact else "fast"] = out
    print("exact" if exact else "fast", json.dumps(out))
lib.gs_set_exact_exp(0)
res["group_channels"] = G
res["note"] = ("median over %d warm calls of the summed us of a kernel name's launches in one call (HIP events of the "
               "library's launch profile), C3 view: 1M Gaussians SH3 1920x1080, identity camera, seed 0" % N)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
