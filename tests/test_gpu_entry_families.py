"""Every narrow C entry against the widest entry of its family, bit for bit.

The Python bridge and the torch extension call only the widest entry of each family
(gs_backward_accumulate_absgrad, gs_backward_camera_aa, gs_backward_render_aux, gs_forward_preprocess_aa,
gs_forward_render_aux, gs_backward_gaussians_range, gs_backward_gaussians_adam_stats_aux); the narrow
entries stay in the library for C callers, as forwarders
with NULL / 0 in the slots they lack (csrc/gs_api.hip).  Here each narrow entry and its widest one are
called directly through _native.load() on the same inputs and fresh outputs: `widen` hands the wide entry
the narrow call's values by parameter name and NULL / 0 for every parameter the narrow one does not have.

Scene: 300 Gaussians (two 256-row blocks, the second ragged) on a 40 x 24 image (ragged 16 x 16 tiles),
degree 3, M = 16, scales and rotations; a third of the rows lie behind the camera or off screen.  Colours
as whole SH rows, split rows, or precomputed.
"""
import ctypes
import math

import pytest
import torch

import gs_scenes
from diff_gaussian_rasterization import _native

pytestmark = pytest.mark.gpu

P, W, H = 300, 40, 24
GS_ACC_OPACITY, GS_ACC_MEANS3D = 4, 8
GRAD_WIDTHS = dict(dL_dmeans2D=3, dL_dcolors=3, dL_dopacity=1, dL_dmeans3D=3, dL_dcov3D=6, dL_dsh=48, dL_dscales=3,
                   dL_drotations=4)
WIDEST_BACKWARD = "gs_backward_accumulate_absgrad"


def names(entry):
    return [n for n, _ in _native.ENTRIES[entry][1]]


def call(lib, entry, vals):
    """entry(...) with each of its parameters taken from vals by name; a tensor goes as its address."""
    args = {n: ctypes.c_void_p(vals[n].data_ptr()) if torch.is_tensor(vals[n]) else vals[n] for n in names(entry)}
    rc = getattr(lib, entry)(*_native.ordered(entry, **args))
    assert rc == 0, (entry, _native.last_error())


def widen(narrow, wide, vals):
    """The wide entry's arguments that stand for narrow(**vals): the same value under the same name
    (a wide entry without shs_dc takes it as shs, as the _split forwarder passes it), NULL / 0 in every other
    slot."""
    dc = "shs_dc" if "shs_dc" in names(wide) else "shs"
    have = {(dc if n == "shs_dc" else n): vals[n] for n in names(narrow)}
    assert set(have) <= set(names(wide)), (narrow, wide)
    return {n: have.get(n, 0 if t in (ctypes.c_int, ctypes.c_uint) else None) for n, t in _native.ENTRIES[wide][1]}


def same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), what


def u8(n, dev):
    return torch.zeros((int(n),), dtype=torch.uint8, device=dev)


def run_pair(lib, narrow, wide, make, after=None, **fixed):
    """narrow(...) and wide(widen(...)) on make()'s values (same contents, fresh buffers each time);
    make() -> (values by name, {name: output tensor}); after(values, outputs): further calls on the pair's
    own buffers that add outputs; fixed: what the narrow entry's forwarder passes in a slot other than
    NULL / 0.  Every output must agree bit for bit."""
    outs = []
    for entry in (narrow, wide):
        vals, out = make()
        args = {n: vals[n] for n in names(narrow)}
        call(lib, entry, args if entry == narrow else dict(widen(narrow, wide, args), **fixed))
        if after is not None:
            after(vals, out)
        torch.cuda.synchronize()
        outs.append(out)
    assert outs[0].keys() == outs[1].keys() and outs[0]
    for n in outs[0]:
        same_bits(outs[0][n], outs[1][n], (narrow, wide, n))
    return outs[0]


@pytest.fixture(scope="module")
def lib():
    return _native.load()


@pytest.fixture(scope="module")
def scene(device):
    """{kind: the scene's and camera's arguments by name} for kind in whole / split / precomp."""
    cam = gs_scenes.identity_camera(W, H)
    sc = gs_scenes.random_gaussians(P, 3, cam=cam, seed=5, scale_range=(0.05, 0.4))
    means = sc.means3D.clone()  # (identity camera: world = camera coordinates, z in [2, 10])
    means[0::6, 2] *= -1.0  # behind the camera
    means[3::6, 0] += 50.0  # far off screen
    g = torch.Generator().manual_seed(6)
    d = lambda t: t.contiguous().to(device)  # noqa: E731
    shs = d(sc.shs)
    base = dict(P=P, D=3, M=16, background=d(torch.tensor([0.1, 0.2, 0.3])), image_width=W, image_height=H,
                means3D=d(means), shs=shs, shs_rest=None, colors_precomp=None, opacities=d(sc.opacities),
                scales=d(sc.scales), scale_modifier=1.0, rotations=d(sc.rotations), cov3D_precomp=None,
                viewmatrix=d(cam.world_view_transform), projmatrix=d(cam.full_proj_transform),
                campos=d(cam.camera_center), tan_fovx=math.tan(cam.FoVx / 2), tan_fovy=math.tan(cam.FoVy / 2),
                prefiltered=0, debug=0, stream=ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    dc, rest = d(sc.shs[:, :1]), d(sc.shs[:, 1:])
    return dict(whole=base, split=dict(base, shs=dc, shs_dc=dc, shs_rest=rest),
                precomp=dict(base, D=0, M=0, shs=None, colors_precomp=d(torch.rand((P, 3), generator=g))))


@pytest.fixture(scope="module")
def forwards(lib, scene, device):
    """forward(kind, antialiasing) -> a finished two-call forward of that scene: its buffers by the
    backward entries' parameter names.  Computed once per key; users clone (fresh)."""
    done = {}

    def forward(kind, antialiasing=0):
        if (kind, antialiasing) not in done:
            pool = scene[kind]
            radii = torch.zeros((P,), dtype=torch.int32, device=device)
            geom = u8(lib.gs_geom_buffer_bytes(P), device)
            nr = ctypes.c_longlong(0)
            out = dict(radii_out=radii, geom_buffer=geom)
            if kind == "split":
                call(lib, "gs_forward_preprocess_split", dict(pool, **out, num_rendered=ctypes.byref(nr)))
            else:
                call(lib, "gs_forward_preprocess_aa", dict(pool, **out, num_rendered_host=ctypes.byref(nr),
                                                            antialiasing=antialiasing))
            R = int(nr.value)
            hidden = int((radii == 0).sum())
            assert R > 0 and P // 3 <= hidden < P // 2, (R, hidden)  # invisible rows are exercised
            st = dict(radii=radii, geom_buffer=geom, num_rendered=R,
                      binning_buffer=u8(lib.gs_binning_buffer_bytes(R, W, H), device),
                      image_buffer=u8(lib.gs_image_buffer_bytes(W, H), device))
            call(lib, "gs_forward_render_aux", dict(pool, **st, out_color=torch.empty((3, H, W), device=device),
                                                    out_invdepth=torch.empty((H, W), device=device),
                                                    out_alpha=torch.empty((H, W), device=device)))
            torch.cuda.synchronize()
            done[kind, antialiasing] = st
        return done[kind, antialiasing]

    return forward


def fresh(vals):
    return {n: v.clone() if torch.is_tensor(v) else v for n, v in vals.items()}


def backward_values(lib, scene, forwards, device, kind, antialiasing=0, aux=False, accumulate=0):
    """make() of a per-view backward: the scene, a fresh copy of its forward, dL/dpixel, prefilled gradient
    outputs (the same random values each time: an accumulating bit adds to them) and a scratch."""
    st = forwards(kind, antialiasing)
    g = torch.Generator().manual_seed(11)
    dpix = (1e-2 * torch.randn((3, H, W), generator=g)).to(device)
    daux = [(1e-2 * torch.randn((H, W), generator=g)).to(device) for _ in range(2)]
    fill = {n: torch.randn((P, w), generator=g).to(device) for n, w in GRAD_WIDTHS.items()}
    R = st["num_rendered"]
    n_scratch = max(lib.gs_grad_buffer_bytes(R), lib.gs_grad_buffer_bytes_aux(R, P),
                    lib.gs_grad_buffer_bytes_absgrad(R, P))

    def make():
        grads = fresh(fill)
        if kind == "split":
            grads["dL_dcolors"] = None  # SH colours: the _split entry has no such output
        if kind == "precomp":
            grads["dL_dsh"] = None
        vals = dict(scene[kind], **fresh(st), **grads, dL_dout_color=dpix,
                    dL_dout_invdepth=daux[0] if aux else None, dL_dout_alpha=daux[1] if aux else None,
                    grad_buffer=u8(n_scratch, device), accumulate=accumulate, wait_event=None,
                    antialiasing=antialiasing, dL_dmeans2D_abs=None)
        return vals, {n: t for n, t in grads.items() if t is not None}

    return make, fill


ACC = GS_ACC_OPACITY | GS_ACC_MEANS3D
BACKWARDS = [("gs_backward", "whole", {}), ("gs_backward", "precomp", {}),
             ("gs_backward_accumulate", "whole", dict(accumulate=ACC)),
             ("gs_backward_accumulate", "precomp", dict(accumulate=ACC)),
             ("gs_backward_accumulate_aux", "whole", dict(accumulate=ACC, aux=True)),
             ("gs_backward_accumulate_aux", "split", dict(accumulate=ACC, aux=True)),
             ("gs_backward_accumulate_aux", "precomp", dict(aux=True)),
             ("gs_backward_accumulate_aa", "whole", dict(accumulate=ACC, antialiasing=1)),
             ("gs_backward_accumulate_aa", "precomp", dict(antialiasing=1, aux=True)),
             ("gs_backward_accumulate_split", "split", dict(accumulate=ACC))]


@pytest.mark.parametrize("entry,kind,how", BACKWARDS, ids=[f"{e[3:]}-{k}" for e, k, _ in BACKWARDS])
def test_per_view_backward(lib, scene, forwards, device, entry, kind, how):
    make, fill = backward_values(lib, scene, forwards, device, kind, **how)
    out = run_pair(lib, entry, WIDEST_BACKWARD, make)
    assert len(out) == (7 if kind != "whole" else 8)
    # the gradients are real: visible rows were written, and an accumulating output kept its prefill
    visible = forwards(kind, how.get("antialiasing", 0))["radii"] > 0
    assert bool((out["dL_dmeans3D"][visible] != fill["dL_dmeans3D"][visible]).any())
    assert bool((out["dL_dscales"][visible] != 0).any())
    if how.get("accumulate"):
        assert torch.equal(out["dL_dopacity"][~visible], fill["dL_dopacity"][~visible])
    else:
        assert bool((out["dL_dopacity"][~visible] == 0).all())


@pytest.mark.parametrize("kind", ["whole", "precomp"])
def test_camera_gradients(lib, scene, forwards, device, kind):
    make_backward, _ = backward_values(lib, scene, forwards, device, kind)

    def make():  # the camera entries read the record sums a backward of the view left in its geometry buffer
        vals, _ = make_backward()
        call(lib, WIDEST_BACKWARD, vals)
        cam = dict(dL_dviewmatrix=torch.full((16,), 7.0, device=device),
                   dL_dprojmatrix=torch.full((16,), 7.0, device=device),
                   dL_dcampos=torch.full((3,), 7.0, device=device))
        return dict(vals, **cam, aux_grad_buffer=None, aux_valid=0,
                    scratch=u8(lib.gs_camera_grad_scratch_bytes(P), device)), cam

    out = run_pair(lib, "gs_backward_camera", "gs_backward_camera_aa", make)
    assert bool((out["dL_dviewmatrix"] != 7.0).all()) and bool((out["dL_dviewmatrix"][:12] != 0).any())


@pytest.mark.parametrize("kind", ["whole", "precomp"])
def test_render_half(lib, scene, forwards, device, kind):
    """gs_backward_render against gs_backward_render_aux with NULL aux gradients and sums: the view's
    dL_dmeans2D, then the outputs of one gs_backward_gaussians pass over each one's geometry buffer."""
    make_backward, _ = backward_values(lib, scene, forwards, device, kind)
    keep = []

    def make():
        vals, grads = make_backward()
        return dict(vals, invdepth_sums=None), grads

    def after(vals, out):
        view = _native.ViewGrad(*(vals[n].data_ptr() for n in ("viewmatrix", "projmatrix", "campos")), vals["tan_fovx"],
                                vals["tan_fovy"], W, H, vals["geom_buffer"].data_ptr())
        keep.append(view)
        call(lib, "gs_backward_gaussians", dict(vals, num_views=1, views=ctypes.byref(view)))

    out = run_pair(lib, "gs_backward_render", "gs_backward_render_aux", make, after)
    assert bool((out["dL_dmeans2D"] != 0).any()) and bool((out["dL_dmeans3D"] != 0).any())


@pytest.mark.parametrize("kind", ["whole", "precomp"])
def test_preprocess(lib, scene, device, kind):
    """gs_forward_preprocess against gs_forward_preprocess_aa(..., 0): num_rendered, the radii, and the image
    gs_forward_render composites from each (the raw geometry buffer has padding nobody writes)."""
    counts = []

    def make():
        nr = ctypes.c_longlong(-1)
        counts.append(nr)
        out = dict(radii_out=torch.full((P,), -1, dtype=torch.int32, device=device))
        return dict(scene[kind], **out, geom_buffer=u8(lib.gs_geom_buffer_bytes(P), device),
                    num_rendered_host=ctypes.byref(nr)), out

    def after(vals, out):
        R = int(counts[-1].value)
        assert R > 0
        out["image"] = torch.empty((3, H, W), device=device)
        call(lib, "gs_forward_render", dict(vals, radii=vals["radii_out"], num_rendered=R, out_color=out["image"],
                                            binning_buffer=u8(lib.gs_binning_buffer_bytes(R, W, H), device),
                                            image_buffer=u8(lib.gs_image_buffer_bytes(W, H), device)))

    out = run_pair(lib, "gs_forward_preprocess", "gs_forward_preprocess_aa", make, after)
    assert counts[0].value == counts[1].value
    assert bool((out["radii_out"] >= 0).all()) and bool((out["image"] != out["image"][:, :1, :1]).any())


@pytest.mark.parametrize("kind", ["whole", "precomp"])
def test_render(lib, scene, device, kind):
    """gs_forward_render against gs_forward_render_aux with NULL planes, each behind a preprocess of its own:
    the image."""
    def make():
        nr = ctypes.c_longlong(-1)
        radii = torch.zeros((P,), dtype=torch.int32, device=device)
        geom = u8(lib.gs_geom_buffer_bytes(P), device)
        call(lib, "gs_forward_preprocess_aa", dict(scene[kind], radii_out=radii, geom_buffer=geom,
                                                    num_rendered_host=ctypes.byref(nr), antialiasing=0))
        R = int(nr.value)
        assert R > 0
        out = dict(out_color=torch.full((3, H, W), 7.0, device=device))
        return dict(scene[kind], **out, radii=radii, geom_buffer=geom, num_rendered=R,
                    binning_buffer=u8(lib.gs_binning_buffer_bytes(R, W, H), device),
                    image_buffer=u8(lib.gs_image_buffer_bytes(W, H), device)), out

    out = run_pair(lib, "gs_forward_render", "gs_forward_render_aux", make)
    image = out["out_color"]
    assert bool((image != 7.0).all()) and bool((image != image[:, :1, :1]).any())


@pytest.mark.parametrize("kind", ["whole", "precomp"])
def test_per_gaussian_half(lib, scene, forwards, device, kind):
    """gs_backward_gaussians against gs_backward_gaussians_range(first = 0, count = P) behind a per-tile half
    of its own, two outputs accumulating over their prefill."""
    make_backward, fill = backward_values(lib, scene, forwards, device, kind, accumulate=ACC)
    keep = []

    def make():
        vals, grads = make_backward()
        call(lib, "gs_backward_render_aux", dict(vals, accumulate=0, invdepth_sums=None))
        view = _native.ViewGrad(*(vals[n].data_ptr() for n in ("viewmatrix", "projmatrix", "campos")), vals["tan_fovx"],
                                vals["tan_fovy"], W, H, vals["geom_buffer"].data_ptr())
        keep.append(view)
        del grads["dL_dmeans2D"]  # the per-tile half's output
        return dict(vals, num_views=1, views=ctypes.byref(view)), grads

    out = run_pair(lib, "gs_backward_gaussians", "gs_backward_gaussians_range", make, count=P)
    visible = forwards(kind)["radii"] > 0
    assert bool((out["dL_dscales"][visible] != 0).any())
    assert torch.equal(out["dL_dopacity"][~visible], fill["dL_dopacity"][~visible])


@pytest.mark.parametrize("entry", ["gs_backward_gaussians_adam", "gs_backward_gaussians_adam_stats"])
def test_fused_adam(lib, scene, forwards, device, entry):
    """One fused backward + Adam step from cloned parameters and moments: the narrow entry against
    gs_backward_gaussians_adam_stats_aux with NULL statistics / inverse-depth sums."""
    pool = scene["split"]
    make_backward, _ = backward_values(lib, scene, forwards, device, "split")
    vals, grads = make_backward()  # the per-tile half leaves the view's record sums in its geometry buffer
    call(lib, "gs_backward_render_aux", dict(vals, invdepth_sums=None))
    torch.cuda.synchronize()
    geom, grad2d, radii = vals["geom_buffer"], grads["dL_dmeans2D"], vals["radii"]
    g = torch.Generator().manual_seed(13)
    # raw parameters in group order; the forward read their activations (scales, rotations: the scene's)
    params = [pool["means3D"], pool["shs_dc"], pool["shs_rest"], torch.logit(pool["opacities"]),
              torch.log(pool["scales"]), 1.7 * pool["rotations"]]
    exp_avg = [(1e-3 * torch.randn(p.shape, generator=g)).to(device) for p in params]
    exp_avg_sq = [(1e-6 * torch.rand(p.shape, generator=g)).to(device) for p in params]
    stats = dict(max_radii2D=torch.rand((P,), generator=g).to(device),
                 grad_accum=torch.rand((P, 1), generator=g).to(device), denom=torch.zeros((P, 1), device=device))
    keep = []

    def host(ts):
        return ctypes.cast((ctypes.c_void_p * 6)(*[t.data_ptr() for t in ts]), ctypes.c_void_p)

    def make():
        p, m, v, s = ([t.clone() for t in ts] for ts in (params, exp_avg, exp_avg_sq, list(stats.values())))
        gb = geom.clone()
        view = _native.ViewGrad(*(pool[n].data_ptr() for n in ("viewmatrix", "projmatrix", "campos")),
                                pool["tan_fovx"], pool["tan_fovy"], W, H, gb.data_ptr())
        hyper = ((ctypes.c_double * 6)(1.6e-4, 2.5e-3, 1.25e-4, 5e-2, 5e-3, 1e-3), (ctypes.c_longlong * 6)(*[3] * 6))
        keep.extend([gb, view, hyper])
        out = dict(zip(stats, s))
        for k, group in enumerate(zip(p, m, v)):
            out.update({f"{what}{k}": t for what, t in zip(("param", "exp_avg", "exp_avg_sq"), group)})
        return dict(P=P, D=3, M=16, means3D=p[0], shs_dc=p[1], shs_rest=p[2], scales=pool["scales"], scale_modifier=1.0,
                    rotations=pool["rotations"], view=ctypes.byref(view), params_host=host(p), exp_avg_host=host(m),
                    exp_avg_sq_host=host(v), lr_host=ctypes.cast(hyper[0], ctypes.c_void_p),
                    step_host=ctypes.cast(hyper[1], ctypes.c_void_p), weight_decay_host=None, beta1=0.9, beta2=0.999,
                    eps=1e-15, maximize=0, radii=radii, grad2d=grad2d, grad_stride=3, debug=0, stream=pool["stream"],
                    **dict(zip(stats, s))), out

    out = run_pair(lib, entry, "gs_backward_gaussians_adam_stats_aux", make)
    visible = radii > 0
    for k in range(6):
        assert bool((out[f"param{k}"][visible] != params[k][visible]).any()), k
    with_stats = entry.endswith("_stats")
    assert torch.equal(out["denom"][visible], stats["denom"][visible] + (1 if with_stats else 0))
    assert torch.equal(out["denom"][~visible], stats["denom"][~visible])
