"""Feature rendering (gs_features, gs_feature_forward / gs_feature_backward), the parts that need no GPU.

1-2. The dense reference (tests/dense_ref_features.py) checks itself in fp64 on the `sparse` scene of
     tests/test_gpu_contrib.py: with features = colours its `out` is dense_ref.render's image over a zero
     background, and its `dfeat` is the gradient of sum(g * img) with respect to colors_precomp
     (autograd); a column of dfeat is dense_ref_contrib's wsum under that channel's map.
3-6. The header, the signature table, the two entries' host validation (the table idiom of
     tests/test_contrib_cpu.py) and gs_feature_scratch_bytes.
7-8. gs_features' input refusals and its autograd wiring over monkeypatched _C fakes.
"""
import ctypes
import math
import os
import re

import pytest
import torch

import dense_ref
import dense_ref_contrib
import dense_ref_features
import gs_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1-2: the reference checks itself ----
_REF = {}


def _sparse_ref():
    if not _REF:
        W, H, P = 200, 120, 2000
        cam = gs_scenes.identity_camera(W, H)
        sc = gs_scenes.random_gaussians(P, 3, cam=cam, seed=41)
        f = torch.float64
        gen = torch.Generator().manual_seed(3)
        g = torch.randn((3, H, W), generator=gen, dtype=f)
        colors = torch.rand((P, 3), generator=gen, dtype=f).requires_grad_(True)
        geo = dict(scales=sc.scales.to(f), rots=sc.rotations.to(f))
        cams = (cam.world_view_transform.to(f), cam.full_proj_transform.to(f), cam.camera_center.to(f),
                math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), W, H)
        means, m2, op = sc.means3D.to(f), torch.zeros((P, 3), dtype=f), sc.opacities.to(f)
        img, radii = dense_ref.render(means, m2, op, *cams, torch.zeros(3, dtype=f), colors=colors, **geo)
        (grad,) = torch.autograd.grad((g * img).sum(), colors)
        ref = dense_ref_features.features_local(means, m2, op, *cams, colors.detach(), g=g, colors=colors.detach(),
                                                **geo)
        m = g[1].abs()
        con = dense_ref_contrib.contributions_local(means, m2, op, *cams, weights=m, colors=colors.detach(), **geo)
        ref1 = dense_ref_features.features_local(means, m2, op, *cams, colors.detach()[:, 1:2], g=m[None],
                                                 colors=colors.detach(), **geo)
        _REF.update(img=img.detach(), radii=radii, grad=grad, ref=ref, con=con, ref1=ref1)
    return _REF


def test_reference_out_is_the_image_over_a_zero_background():
    r = _sparse_ref()
    out, img = r["ref"]["out"], r["img"]
    assert torch.equal(r["ref"]["radii"], r["radii"]) and out.shape == img.shape
    d, scale = float((out - img).abs().max()), float(img.abs().max())
    print(f"max|out_ref - image| {d:.3e}, max|image| {scale:.3e}")
    assert scale > 0.1 and d <= 1e-12 * scale
    # one column alone gives that channel
    assert float((r["ref1"]["out"][0] - img[1]).abs().max()) <= 1e-12 * scale


def test_reference_dfeat_is_the_colour_gradient_and_wsum():
    r = _sparse_ref()
    dfeat, grad = r["ref"]["dfeat"], r["grad"]
    scale = float(grad.abs().max())
    d = float((dfeat - grad).abs().max())
    print(f"max|dfeat_ref - dL/dcolors| {d:.3e}, max|ref| {scale:.3e}")
    assert scale > 0 and d <= 1e-12 * scale
    wsum = r["con"]["wsum"]
    assert float((r["ref1"]["dfeat"][:, 0] - wsum).abs().max()) <= 1e-12 * float(wsum.max())
    assert torch.equal(r["ref"]["flag"], r["con"]["flag"])


# ---- 3-6: the C entries' host contract ----
def _header():
    return open(os.path.join(ROOT, "include", "gsrast.h")).read()


def test_header_defines_has_features_and_keeps_abi_17():
    import gs_features

    h = _header()
    assert re.search(r"#define GSRAST_HAS_FEATURES 1\b", h)
    assert re.search(r"#define GSRAST_ABI_VERSION 17\b", h)
    cmax = int(re.search(r"#define GS_MAX_FEATURE_CHANNELS (\d+)", h).group(1))
    assert cmax >= 512 and cmax == gs_features.MAX_CHANNELS
    assert "not defined for the bounded forwards" in h.split("GSRAST_HAS_FEATURES, an extension")[1]


def test_entries_are_in_the_table_and_in_the_library():
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    for name in ("gs_feature_group_channels", "gs_feature_scratch_bytes", "gs_feature_forward", "gs_feature_backward"):
        assert name in _native.SIGNATURES
        assert getattr(lib, name) is not None
        assert re.search(r"\b%s\(" % name, _header())
    G = lib.gs_feature_group_channels()
    assert G >= 1 and G == lib.gs_feature_group_channels()


_BUF = (ctypes.c_float * 64)()  # host words; never dereferenced by a row
X = ctypes.cast(_BUF, ctypes.c_void_p)
VIEW = "P C W H view proj campos tan_fovx tan_fovy radii geom num_rendered binning image".split()
PARAMS = {
    "gs_feature_forward": VIEW + "features out debug stream".split(),
    "gs_feature_backward": VIEW + "dL_dout scratch dL_dfeatures accumulate debug stream".split(),
}
DEFAULTS = dict(P=4, C=5, W=16, H=16, tan_fovx=0.5, tan_fovy=0.5, num_rendered=10, accumulate=0, debug=0, stream=None)
E_P = "P must be >= 0"
E_C = "feature channels must lie in [1, %d] (got %d)"
E_SIZE = "image size must be positive (got %d x %d)"
E_LIMIT = ("image size %d x %d is too large: at most 65535 tiles of 16 pixels per row and per column and 4194304 "
           "tiles in all")
E_OUT = "missing output pointer"
E_BUF = "missing buffer pointer"
E_NR = "num_rendered out of range"


def _cmax():
    return int(re.search(r"#define GS_MAX_FEATURE_CHANNELS (\d+)", _header()).group(1))


# each row trips one check and every later one: the earlier check's message wins
COMMON = [
    (dict(P=-1, C=0, W=0), lambda: E_P),
    (dict(C=0, W=0), lambda: E_C % (_cmax(), 0)),
    (dict(C=-3, num_rendered=-1), lambda: E_C % (_cmax(), -3)),
    (dict(C=1 << 20, H=0), lambda: E_C % (_cmax(), 1 << 20)),
    (dict(W=0, num_rendered=-1), lambda: E_SIZE % (0, 16)),
    (dict(H=-2, geom=None), lambda: E_SIZE % (16, -2)),
    (dict(W=16 * 65536, num_rendered=-1), lambda: E_LIMIT % (16 * 65536, 16)),
    (dict(W=16 * 4096, H=16 * 1025, geom=None), lambda: E_LIMIT % (16 * 4096, 16 * 1025)),
    (dict(num_rendered=-1, geom=None), lambda: E_NR),
    (dict(num_rendered=1 << 31, binning=None), lambda: E_NR),
    (dict(geom=None), lambda: E_BUF),
    (dict(binning=None), lambda: E_BUF),
    (dict(image=None), lambda: E_BUF),
]
ROWS = [("gs_feature_forward", o, t) for o, t in COMMON] + [
    ("gs_feature_forward", dict(out=None, geom=None), lambda: E_OUT),
    ("gs_feature_forward", dict(P=0, out=None), lambda: E_OUT),  # also for an empty scene
    ("gs_feature_forward", dict(features=None), lambda: E_BUF),
] + [("gs_feature_backward", o, t) for o, t in COMMON] + [
    ("gs_feature_backward", dict(dL_dfeatures=None, geom=None), lambda: E_OUT),
    ("gs_feature_backward", dict(dL_dout=None), lambda: E_BUF),
    ("gs_feature_backward", dict(scratch=None, accumulate=1), lambda: E_BUF),
]


@pytest.mark.parametrize("entry,over,text", ROWS,
                         ids=[f"{i:02d}-{r[0][11:]}-" + ",".join(r[1]) for i, r in enumerate(ROWS)])
def test_feature_entries_early_return(entry, over, text):
    from diff_gaussian_rasterization import _native

    params = PARAMS[entry]
    assert not set(over) - set(params)
    assert len(params) == len(_native.SIGNATURES[entry][1])
    lib = _native.load()
    args = [over[n] if n in over else DEFAULTS.get(n, X) for n in params]
    assert getattr(lib, entry)(*args) == 1
    assert lib.gs_last_error().decode() == text()


@pytest.mark.parametrize("entry", sorted(PARAMS))
def test_channel_limit_is_inclusive(entry):
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    params = PARAMS[entry]
    base = {n: DEFAULTS.get(n, X) for n in params}
    # C == the limit passes the channel check (the next failing check answers); one more does not
    for C, text in ((_cmax(), E_NR), (_cmax() + 1, E_C % (_cmax(), _cmax() + 1))):
        assert getattr(lib, entry)(*[{**base, "C": C, "num_rendered": -1}[n] for n in params]) == 1
        assert lib.gs_last_error().decode() == text


def test_backward_of_an_empty_scene_and_accumulating_without_instances_launch_nothing():
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    params = PARAMS["gs_feature_backward"]
    base = {n: DEFAULTS.get(n, X) for n in params}
    # P == 0: nothing to write; accumulate with no instance: the gradient is left alone (no device call)
    for over in (dict(P=0, geom=None, dL_dfeatures=None), dict(num_rendered=0, accumulate=1, geom=None, scratch=None)):
        assert lib.gs_feature_backward(*[{**base, **over}[n] for n in params]) == 0


def test_scratch_bytes_monotone_multiple_of_256():
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    G = lib.gs_feature_group_channels()
    prev = 0
    for n in (-5, 0, 1, 7, 8, 9, 1000, 12345, 1 << 20, (1 << 31) - 1):
        b = lib.gs_feature_scratch_bytes(n)
        assert b >= 4 * G * max(n, 0) and b >= prev and b > 0 and b % 256 == 0
        assert b < 4 * G * max(n, 1) + 256
        prev = b


# ---- 7-8: gs_features over _C fakes ----
class _Settings:
    image_height, image_width = 24, 40
    tanfovx = tanfovy = 0.5
    bg = torch.zeros(3)
    scale_modifier = 1.0
    viewmatrix = torch.eye(4)
    projmatrix = torch.eye(4)
    sh_degree = 0
    campos = torch.zeros(3)
    prefiltered = False
    debug = False


class _Rasterizer:
    raster_settings = _Settings()


@pytest.fixture
def fakes(monkeypatch):
    """gs_features with a _C whose device calls are host fakes that record their calls"""
    import gs_features

    calls = []
    H, W = _Settings.image_height, _Settings.image_width

    def two_call(bg, means3D, *rest, **kw):
        calls.append(("two_call", kw))
        P = means3D.shape[0]
        u8 = torch.zeros(16, dtype=torch.uint8)
        return 7, torch.zeros((3, H, W)), torch.ones(P, dtype=torch.int32), u8, u8, u8

    def feature_forward(R, radii, geom, binning, img, view, proj, campos, tx, ty, h, w, features, debug=False):
        calls.append(("forward", tuple(features.shape)))
        assert not features.requires_grad
        return features.sum(0)[:, None, None] * torch.ones((features.shape[1], h, w))

    def feature_backward(R, radii, geom, binning, img, view, proj, campos, tx, ty, h, w, dL_dout, debug=False,
                         out=None):
        calls.append(("backward", tuple(dL_dout.shape)))
        return dL_dout.sum((1, 2))[None, :] * torch.ones((radii.numel(), dL_dout.shape[0]))

    def dev_check(t, name):
        calls.append(("dev_check", name))

    monkeypatch.setattr(gs_features._C, "rasterize_gaussians_two_call", two_call)
    monkeypatch.setattr(gs_features._C, "feature_forward", feature_forward)
    monkeypatch.setattr(gs_features._C, "feature_backward", feature_backward)
    monkeypatch.setattr(gs_features._C, "_dev_check", dev_check)
    monkeypatch.setattr(gs_features._C, "check_image_size", lambda W, H: None)
    return gs_features, calls


def _kw(P=6):
    return dict(means3D=torch.zeros((P, 3)), opacities=torch.ones((P, 1)), shs=torch.zeros((P, 1, 3)),
                scales=torch.ones((P, 3)), rotations=torch.ones((P, 4)))


def test_from_inputs_refuses_like_the_rasterizer(fakes):
    gf, calls = fakes
    r, kw = _Rasterizer(), _kw()
    with pytest.raises(Exception, match="Please provide excatly one of either SHs or precomputed colors!"):
        gf.FeatureView.from_inputs(r, **dict(kw, shs=None))
    with pytest.raises(Exception, match="Please provide excatly one of either SHs or precomputed colors!"):
        gf.FeatureView.from_inputs(r, **dict(kw, colors_precomp=torch.zeros((6, 3))))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        gf.FeatureView.from_inputs(r, **dict(kw, scales=None))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        gf.FeatureView.from_inputs(r, **dict(kw, cov3D_precomp=torch.zeros((6, 6))))
    assert not calls  # refused before any library call
    v = gf.FeatureView.from_inputs(r, antialiasing=True, **kw)
    assert [c[0] for c in calls] == ["dev_check", "two_call"] and calls[1][1] == dict(antialiasing=True)
    assert v.num_rendered == 7 and v.radii.shape == (6,) and v.color.shape == (3, 24, 40)
    assert (v.image_height, v.image_width) == (24, 40)


def test_render_features_refuses_and_launches_nothing(fakes):
    gf, calls = fakes
    v = gf.FeatureView.from_inputs(_Rasterizer(), **_kw())
    del calls[:]
    bad = [torch.zeros((6,)), torch.zeros((5, 4)), torch.zeros((6, 4, 1)), torch.zeros((6, 0)),
           torch.zeros((6, gf.MAX_CHANNELS + 1)), torch.zeros((6, 4), dtype=torch.float64),
           torch.zeros((6, 4), dtype=torch.float16), torch.zeros((6, 4), device="meta"), [[0.0] * 4] * 6, None]
    for f in bad:
        with pytest.raises(ValueError, match=r"features must be a float32 tensor of shape \(6, C\), 1 <= C <= %d"
                           % gf.MAX_CHANNELS):
            gf.render_features(v, f)
    assert not calls


def test_render_features_autograd_wiring(fakes):
    gf, calls = fakes
    v = gf.FeatureView.from_inputs(_Rasterizer(), **_kw())
    del calls[:]
    f = torch.arange(24, dtype=torch.float32).reshape(6, 4).requires_grad_(True)
    out = gf.render_features(v, f)
    assert out.shape == (4, 24, 40) and out.requires_grad
    (out * 2.0).sum().backward()
    assert calls == [("forward", (6, 4)), ("backward", (4, 24, 40))]
    assert f.grad.shape == (6, 4) and torch.equal(f.grad, torch.full((6, 4), 2.0 * 24 * 40))
    # the same view again with another C; no graph without a leaf that wants one
    out1 = gf.render_features(v, torch.ones((6, 1)))
    assert out1.shape == (1, 24, 40) and not out1.requires_grad
    # the one-shot convenience
    out2 = gf.render_features_for(_Rasterizer(), torch.ones((6, 9)), **_kw())
    assert out2.shape == (9, 24, 40)
