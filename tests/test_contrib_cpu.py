"""Contribution statistics and importance pruning, the parts that need no GPU.

1-3. The dense reference (tests/dense_ref_contrib.py) checks itself in fp64 on the `sparse` scene of
     tests/test_gpu_aux.py: wsum is the gradient of sum_p m_p img[0, p] with respect to
     colors_precomp[:, 0] of dense_ref.render (autograd), the sum of wsum telescopes to
     sum_p m_p alpha_p, and count == 0 <=> wmax == 0.
4-5. gs_contrib_stats' host validation (the table idiom of tests/test_camera_cpu.py) and
     gs_contrib_scratch_bytes.
6.   gs_importance.keep_mask: each threshold, their conjunction, keep_fraction with ties.
7.   gs_importance.prune on CPU tensors against direct indexing.
"""
import ctypes
import math
import os
import re

import pytest
import torch

import dense_ref
import dense_ref_contrib
import gs_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1-3: the reference checks itself ----
_REF = {}


def _sparse_ref():
    if not _REF:
        W, H = 200, 120
        cam = gs_scenes.identity_camera(W, H)
        sc = gs_scenes.random_gaussians(2000, 3, cam=cam, seed=41)
        f = torch.float64
        g = torch.Generator().manual_seed(3)
        m = torch.rand((H, W), generator=g, dtype=f)
        m[5:9, 20:90] = 0.0  # masked pixels
        colors = torch.rand((2000, 3), generator=g, dtype=f).requires_grad_(True)
        geo = dict(scales=sc.scales.to(f), rots=sc.rotations.to(f))
        cams = (cam.world_view_transform.to(f), cam.full_proj_transform.to(f), cam.camera_center.to(f),
                math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), W, H)
        means, m2, op = sc.means3D.to(f), torch.zeros((2000, 3), dtype=f), sc.opacities.to(f)
        img, radii = dense_ref.render(means, m2, op, *cams, torch.zeros(3, dtype=f), colors=colors, **geo)
        (grad,) = torch.autograd.grad((m * img[0]).sum(), colors)
        ref = dense_ref_contrib.contributions_local(means, m2, op, *cams, weights=m, colors=colors.detach(), **geo)
        _REF.update(m=m, grad=grad, ref=ref, radii=radii)
    return _REF


def test_reference_wsum_is_the_colour_gradient():
    r = _sparse_ref()
    wsum, g = r["ref"]["wsum"], r["grad"][:, 0]
    assert torch.equal(r["ref"]["radii"], r["radii"])
    assert float(g.abs().max()) > 0
    d = float((wsum - g).abs().max())
    print(f"max|wsum_ref - dL/dcolors[:, 0]| {d:.3e}, max|ref| {float(g.abs().max()):.3e}")
    assert bool(((wsum - g).abs() <= 1e-12 * g.abs().max()).all())
    assert bool((r["grad"][:, 1:] == 0).all())


def test_reference_wsum_telescopes_to_alpha():
    r = _sparse_ref()
    total, want = float(r["ref"]["wsum"].sum()), float((r["m"] * r["ref"]["alpha"]).sum())
    assert want > 0 and abs(total - want) <= 1e-12 * want


def test_reference_count_zero_iff_wmax_zero():
    ref = _sparse_ref()["ref"]
    # (a positive weight wherever the map is not masked: a hit under a non-zero weight has w > 0)
    assert torch.equal(ref["count"] == 0, ref["wmax"] == 0)
    assert int((ref["count"] > 0).sum()) > 100 and int((ref["count"] == 0).sum()) > 0
    assert bool((ref["radii"][ref["count"] > 0] > 0).all())


# ---- 4-5: the C entry's host contract ----
def test_header_defines_has_contrib_and_keeps_abi_17():
    h = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    assert re.search(r"#define GSRAST_HAS_CONTRIB 1\b", h)
    assert re.search(r"#define GSRAST_ABI_VERSION 17\b", h)
    assert "The entry that stops a pixel" in h and "is not composited" in h


_BUF = (ctypes.c_float * 64)()  # host words; never dereferenced by a row
X = ctypes.cast(_BUF, ctypes.c_void_p)
PARAMS = ("P W H view proj campos tan_fovx tan_fovy radii geom num_rendered binning image weights scratch wsum wmax "
          "count accumulate debug stream").split()
DEFAULTS = dict(P=4, W=16, H=16, tan_fovx=0.5, tan_fovy=0.5, num_rendered=10, weights=None, accumulate=0, debug=0,
                stream=None)
E_P = "P must be >= 0"
E_SIZE = "image size must be positive (got %d x %d)"
E_LIMIT = ("image size %d x %d is too large: at most 65535 tiles of 16 pixels per row and per column and 4194304 "
           "tiles in all")
E_OUT = "missing output pointer"
E_BUF = "missing buffer pointer"
E_NR = "num_rendered out of range"
ROWS = [
    (dict(P=-1, W=0), E_P),
    (dict(W=0, geom=None), E_SIZE % (0, 16)),
    (dict(H=-2, wsum=None, wmax=None, count=None), E_SIZE % (16, -2)),
    (dict(W=16 * 65536, geom=None), E_LIMIT % (16 * 65536, 16)),
    (dict(W=16 * 4096, H=16 * 1025, geom=None), E_LIMIT % (16 * 4096, 16 * 1025)),
    (dict(wsum=None, wmax=None, count=None, geom=None), E_OUT),
    (dict(P=0, wsum=None, wmax=None, count=None), E_OUT),  # also for an empty scene
    (dict(num_rendered=-1, geom=None), E_NR),
    (dict(num_rendered=1 << 31), E_NR),
    (dict(geom=None), E_BUF),
    (dict(binning=None, wsum=None), E_BUF),
    (dict(image=None, wmax=None, count=None), E_BUF),
    (dict(scratch=None, accumulate=1), E_BUF),
]


@pytest.mark.parametrize("over,text", ROWS, ids=[f"{i:02d}-" + ",".join(r[0]) for i, r in enumerate(ROWS)])
def test_contrib_stats_early_return(over, text):
    from diff_gaussian_rasterization import _native

    assert not set(over) - set(PARAMS)
    assert len(PARAMS) == len(_native.SIGNATURES["gs_contrib_stats"][1])
    lib = _native.load()
    args = [over[n] if n in over else DEFAULTS.get(n, X) for n in PARAMS]
    assert lib.gs_contrib_stats(*args) == 1
    assert lib.gs_last_error().decode() == text


def test_contrib_stats_empty_scene_and_accumulating_without_instances_launch_nothing():
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    base = {n: DEFAULTS.get(n, X) for n in PARAMS}
    # P == 0: nothing to write; accumulate with no instance: the outputs are left alone (no device call)
    for over in (dict(P=0, geom=None), dict(num_rendered=0, accumulate=1, geom=None, scratch=None)):
        assert lib.gs_contrib_stats(*[{**base, **over}[n] for n in PARAMS]) == 0


def test_scratch_bytes_monotone_and_at_least_12_per_instance():
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    prev = 0
    for n in (-5, 0, 1, 21, 22, 1000, 12345, 1 << 20, (1 << 31) - 1):
        b = lib.gs_contrib_scratch_bytes(n)
        assert b >= 12 * max(n, 0) and b >= prev and b > 0
        prev = b


# ---- 6: keep_mask ----
def _stats(wsum, wmax, count):
    import gs_importance

    f32, i32 = torch.float32, torch.int32
    return gs_importance.Contributions(torch.tensor(wsum, dtype=f32), torch.tensor(wmax, dtype=f32),
                                       torch.tensor(count, dtype=i32), torch.zeros(len(wsum), dtype=i32))


def test_keep_mask_thresholds_and_fraction():
    import gs_importance as gi

    st = _stats([0.0, 2.0, 0.5, 2.0, 0.5, 0.1], [0.0, 0.9, 0.02, 0.5, 0.3, 0.01], [0, 40, 1, 7, 3, 2])
    T, F = True, False
    assert gi.keep_mask(st).tolist() == [T] * 6
    assert gi.keep_mask(st, min_count=1).tolist() == [F, T, T, T, T, T]
    assert gi.keep_mask(st, min_count=3).tolist() == [F, T, F, T, T, F]
    assert gi.keep_mask(st, min_wmax=0.02).tolist() == [F, T, T, T, T, F]
    assert gi.keep_mask(st, min_count=3, min_wmax=0.4).tolist() == [F, T, F, T, F, F]
    # the top ceil(f P) by wsum, ties by the lower index: 2.0 (1), 2.0 (3), 0.5 (2), 0.5 (4), 0.1, 0.0
    assert gi.keep_mask(st, keep_fraction=0.5).tolist() == [F, T, T, T, F, F]
    assert gi.keep_mask(st, keep_fraction=0.17).tolist() == [F, T, F, T, F, F]  # ceil(1.02) = 2
    assert gi.keep_mask(st, keep_fraction=1 / 6).tolist() == [F, T, F, F, F, F]
    assert gi.keep_mask(st, keep_fraction=0.0).tolist() == [F] * 6
    assert gi.keep_mask(st, keep_fraction=1.0).tolist() == [T] * 6
    assert gi.keep_mask(st, keep_fraction=0.5, score="wmax").tolist() == [F, T, F, T, T, F]
    assert gi.keep_mask(st, keep_fraction=0.5, score="count").tolist() == [F, T, F, T, T, F]
    # ANDed with the thresholds
    assert gi.keep_mask(st, keep_fraction=0.5, min_count=7).tolist() == [F, T, F, T, F, F]
    with pytest.raises(ValueError):
        gi.keep_mask(st, keep_fraction=1.5)
    with pytest.raises(ValueError):
        gi.keep_mask(st, keep_fraction=0.5, score="radii")


# ---- 7: prune ----
_NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
_ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
_SHAPES = ((3,), (1, 3), (15, 3), (1,), (3,), (4,))


class _Model:
    def __init__(self, P, with_state, seed=0):
        g = torch.Generator().manual_seed(seed)
        for a, s in zip(_ATTRS, _SHAPES):
            setattr(self, a, torch.nn.Parameter(torch.randn((P,) + s, generator=g)))
        self.optimizer = torch.optim.Adam([{"params": [getattr(self, a)], "lr": 1e-3 * (k + 1), "name": n}
                                           for k, (a, n) in enumerate(zip(_ATTRS, _NAMES))], eps=1e-15)
        if with_state:
            for a in _ATTRS:
                getattr(self, a).grad = torch.randn(getattr(self, a).shape, generator=g)
            self.optimizer.step()
            self.optimizer.step()
        self.xyz_gradient_accum = torch.rand((P, 1), generator=g)
        self.denom = torch.rand((P, 1), generator=g)
        self.max_radii2D = torch.rand((P,), generator=g)


@pytest.mark.parametrize("with_state", [True, False], ids=["adam-state", "no-state"])
def test_prune_matches_direct_indexing(with_state):
    import gs_importance as gi

    P = 37
    m = _Model(P, with_state)
    keep = torch.rand(P, generator=torch.Generator().manual_seed(5)) < 0.6
    assert 0 < int(keep.sum()) < P
    want = {a: getattr(m, a).detach().clone()[keep] for a in _ATTRS}
    old = {a: getattr(m, a) for a in _ATTRS}
    moments = {a: {k: (v.clone()[keep] if k != "step" else v.clone()) for k, v in m.optimizer.state[old[a]].items()}
               for a in _ATTRS} if with_state else None
    stats = [getattr(m, n).clone()[keep] for n in ("xyz_gradient_accum", "denom", "max_radii2D")]
    gi.prune(m, keep)
    groups = {g["name"]: g for g in m.optimizer.param_groups}
    for k, (a, n) in enumerate(zip(_ATTRS, _NAMES)):
        p = getattr(m, a)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p is not old[a]
        assert torch.equal(p.detach(), want[a])
        assert len(groups[n]["params"]) == 1 and groups[n]["params"][0] is p
        assert groups[n]["lr"] == 1e-3 * (k + 1)
        assert old[a] not in m.optimizer.state
        if with_state:
            st = m.optimizer.state[p]
            assert torch.equal(st["exp_avg"], moments[a]["exp_avg"])
            assert torch.equal(st["exp_avg_sq"], moments[a]["exp_avg_sq"])
            assert float(st["step"]) == float(moments[a]["step"]) == 2.0
        else:
            assert p not in m.optimizer.state
    for got, ref in zip((m.xyz_gradient_accum, m.denom, m.max_radii2D), stats):
        assert torch.equal(got, ref)
    # the optimizer still steps the new parameters
    for a in _ATTRS:
        getattr(m, a).grad = torch.ones_like(getattr(m, a))
    m.optimizer.step()
    assert not torch.equal(m._xyz.detach(), want["_xyz"])


def test_prune_refuses_a_wrong_mask():
    import gs_importance as gi

    m = _Model(9, False)
    for bad in (torch.ones(8, dtype=torch.bool), torch.ones(9, dtype=torch.uint8), torch.ones((9, 1), dtype=torch.bool),
                [True] * 9):
        with pytest.raises(ValueError):
            gi.prune(m, bad)
    assert m._xyz.shape[0] == 9
