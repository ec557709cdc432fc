"""The autograd layer of diff_gaussian_rasterization, as a contract that needs no GPU: which native
call each public call makes, with which objects, and where each gradient ends up.

_C.rasterize_gaussians, _C.rasterize_gaussians_aux, _C.backward_impl and _C.backward_render are
replaced by recording fakes that return CPU tensors of the right shapes, every gradient filled with
a constant of its own; GaussianRasterizer then runs forward and backward on CPU tensors (P = 5,
4 x 6 pixels, M = 16).  Nothing in torch is patched.

The product of cases: call kind (plain, aux_outputs, camera_grads, both) x colour source x covariance
source x sh_split (where the kind allows it) x inputs requiring grad (all, means3D only, none) x
outputs reaching the loss x owner (none, a deferring owner on every parameter input, the same with
opacities left out).  Owners that claim buffers need a device stream: tests/test_gpu_aux.py,
tests/test_gpu_camera.py, tests/test_view_parallel.py.
"""
import itertools
import math

import pytest
import torch

import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import (GaussianRasterizationSettings, GaussianRasterizer, register_gradient_sink,
                                         unregister_gradient_sink)

P, H, W, M, DEG = 5, 4, 6, 16, 3
NUM_RENDERED = 7
TANX, TANY, SCALE_MOD = 0.5, 0.75, 1.25
# the fakes' constants: backward_impl's gradients by name, its camera triple, backward_render's dL/dmeans2D
GRAD = dict(means2D=2.0, colors=3.0, opacity=4.0, means3D=5.0, cov3D=6.0, sh=7.0, scales=8.0, rotations=9.0)
CAM = (11.0, 12.0, 13.0)
DM2 = 21.0
W_COLOR, W_INV, W_ALPHA = 0.5, 0.25, 0.125
# autograd input slot -> (keyword of GaussianRasterizer.forward, gradient name): the package's _SINK_INPUTS order
SLOTS = (("means3D", "means3D"), ("means2D", "means2D"), ("shs", "sh"), ("colors_precomp", "colors"),
         ("opacities", "opacity"), ("scales", "scales"), ("rotations", "rotations"), ("cov3D_precomp", "cov3D"))
GRAD_SHAPE = dict(means2D=(P, 3), colors=(P, 3), opacity=(P, 1), means3D=(P, 3), cov3D=(P, 6), sh=(P, M, 3),
                  scales=(P, 3), rotations=(P, 4))

T_CARRIER = "sh_split: shs must be the [P, M, 3] gradient carrier of cat(features_dc, features_rest)"
T_SPLIT_PREPARED = "sh_split: not supported with prepared views"
T_CAP_PREPARED = "binning_capacity: not supported with prepared views"
T_AUX_PREPARED = "aux_outputs: not supported with prepared views (prepared=)"
T_AUX_BOUNDED = "aux_outputs: not supported with a bounded forward (binning_capacity=)"
T_AUX_DEFER = ("aux_outputs: an alpha / inverse-depth gradient is not supported with a deferring gradient owner "
               "(GradBucket(defer=True), the fused backward + Adam of gs_train_step)")
T_CAM_DEFER = ("camera_grads: not supported with a deferring gradient owner (GradBucket(defer=True), the fused "
               "backward + Adam of gs_train_step)")
T_SPLIT_DEFER = "sh_split: not supported with a deferring gradient bucket"
T_SPLIT_MODIFIED = ("sh_split: features_dc or features_rest was modified by an inplace operation between the "
                    "forward and the backward")
T_COLOUR = "Please provide excatly one of either SHs or precomputed colors!"
T_COV = "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"


def test_slots_are_the_packages_sink_inputs():
    assert dgr._SINK_INPUTS == tuple((k, name) for k, (_kw, name) in enumerate(SLOTS))
    assert tuple(dgr._C.GRAD_NAMES) == tuple(GRAD)


class Native:
    """Recording fakes of the four native calls."""

    def __init__(self, monkeypatch, fail=None):
        self.calls, self.fail = [], fail
        for name in ("rasterize_gaussians", "rasterize_gaussians_aux", "backward_impl", "backward_render"):
            monkeypatch.setattr(dgr._C, name, getattr(self, name))

    def _record(self, name, a, kw):
        self.calls.append((name, a, kw))
        if self.fail == name:
            raise RuntimeError(f"boom in {name}")

    def _forward(self, name, a, kw):
        self._record(name, a, kw)
        n, h, w = a[1].shape[0], a[12], a[13]
        u8 = lambda k: torch.full((8,), k, dtype=torch.uint8)  # noqa: E731
        self.outs = (NUM_RENDERED, torch.rand((3, h, w)), torch.ones((n,), dtype=torch.int32), u8(1), u8(2), u8(3))
        return self.outs

    def rasterize_gaussians(self, *a, **kw):
        return self._forward("rasterize_gaussians", a, kw)

    def rasterize_gaussians_aux(self, *a, **kw):
        out = self._forward("rasterize_gaussians_aux", a, kw)
        self.outs = out + (torch.rand((1, a[12], a[13])), torch.rand((1, a[12], a[13])))
        return self.outs

    def backward_impl(self, *a, **kw):
        self._record("backward_impl", a, kw)
        n, sh_rest = a[1].shape[0], kw.get("sh_rest")
        m = 1 + sh_rest.shape[1] if sh_rest is not None else (a[13].shape[1] if a[13].numel() else 0)
        shape = dict(GRAD_SHAPE, sh=(n, m, 3))
        # want_all=False: a gradient no input can receive is None
        have = dict(means2D=True, colors=a[3].numel() > 0, opacity=True, means3D=True, cov3D=a[7].numel() > 0,
                    sh=a[13].numel() > 0, scales=a[4].numel() > 0, rotations=a[5].numel() > 0)
        ret = tuple(torch.full(shape[k], GRAD[k]) if have[k] else None for k in GRAD)
        cam = kw.get("camera")
        if cam is not None:
            ret += ((torch.full((4, 4), CAM[0]), torch.full((4, 4), CAM[1]),
                     torch.full((3,), CAM[2]) if cam else None),)
        return ret

    def backward_render(self, *a, **kw):
        self._record("backward_render", a, kw)
        return torch.full((a[7], 3), DM2) if a[14] else None


class Deferrer:
    """What GradBucket(defer=True) and gs_train_step._AdamBackward look like to the rasterizer."""
    defers = True

    def __init__(self, accepts_sh_split=False):
        if accepts_sh_split:
            self.accepts_sh_split = True
        self.forwards, self.claims, self.deferred = [], [], []

    def forwarded(self, geom, n):
        self.forwards.append((geom, n))

    def claim(self, t):
        self.claims.append(t)
        return None  # not deferred: plain autograd

    def defer_view(self, ctx, inputs, view):
        self.deferred.append((inputs, view, list(ctx.sinks), tuple(ctx.needs_input_grad[0:8])))


class _Drop(torch.autograd.Function):
    """Identity whose backward hands back no gradient: the output upstream then receives None."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return None


def _tensors(colour, cov, split, req):
    g = torch.Generator().manual_seed(0)
    t = dict(means3D=torch.randn((P, 3), generator=g), means2D=torch.zeros((P, 3)),
             opacities=torch.rand((P, 1), generator=g))
    if colour == "shs":
        t["shs"] = torch.randn((P, M, 3), generator=g)
    else:
        t["colors_precomp"] = torch.rand((P, 3), generator=g)
    if cov == "scale-rot":
        t["scales"], t["rotations"] = torch.rand((P, 3), generator=g), torch.randn((P, 4), generator=g)
    else:
        t["cov3D_precomp"] = torch.rand((P, 6), generator=g)
    sh_split = None
    if split:
        sh_split = (t["shs"][:, :1].clone(), t["shs"][:, 1:].clone())
    for k, v in t.items():
        v.requires_grad_(req == "all" or (req == "means3D" and k == "means3D"))
    return t, sh_split


def _settings(cam_req=(False, False, False), debug=False):
    g = torch.Generator().manual_seed(1)
    # the reference's Camera keeps world_view_transform as a transposed view: not contiguous
    view = torch.randn((4, 4), generator=g).t()
    proj, campos = torch.randn((4, 4), generator=g), torch.randn((3,), generator=g)
    assert not view.is_contiguous() and proj.is_contiguous()
    for c, r in zip((view, proj, campos), cam_req):
        c.requires_grad_(r)
    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=TANX, tanfovy=TANY,
                                         bg=torch.tensor([0.1, 0.2, 0.3]), scale_modifier=SCALE_MOD, viewmatrix=view,
                                         projmatrix=proj, sh_degree=DEG, campos=campos, prefiltered=False, debug=debug)


def _alias(a, b):
    """a is b, or a detached alias of it (the sh_split rows are detached on the way in)."""
    return a is b or (not a.requires_grad and a.data_ptr() == b.data_ptr() and a.shape == b.shape
                      and a.stride() == b.stride() and a._version == b._version)


def _check_forward_call(call, name, s, t, sh_split, prepared=None, capacity=None):
    got, a, kw = call
    assert got == name
    assert set(kw) <= {"sh_rest", "capacity", "prepared"}
    assert len(a) == 19
    assert a[0] is s.bg and a[1] is t["means3D"] and a[3] is t["opacities"]
    for pos, key in ((2, "colors_precomp"), (4, "scales"), (5, "rotations"), (7, "cov3D_precomp")):
        assert a[pos] is t[key] if key in t else a[pos].numel() == 0, key
    if sh_split is not None:
        assert _alias(a[14], sh_split[0]) and _alias(kw["sh_rest"], sh_split[1])
    else:
        assert a[14] is t["shs"] if "shs" in t else a[14].numel() == 0
        assert kw.get("sh_rest") is None
    assert a[8] is not s.viewmatrix and a[8].is_contiguous() and torch.equal(a[8], s.viewmatrix)
    assert not a[8].requires_grad
    assert a[9] is s.projmatrix and a[16] is s.campos
    assert (a[6], a[10], a[11], a[12], a[13], a[15], a[17], a[18]) == (SCALE_MOD, TANX, TANY, H, W, DEG, False, s.debug)
    assert kw.get("prepared") is prepared and kw.get("capacity") == capacity


def _check_backward_args(a, fwd, s, color_grad):
    """The 21 positional arguments of backward_impl against the forward call's and its outputs."""
    (_n, fa, fkw), outs = fwd
    assert len(a) == 21
    for pos, fpos in ((0, 0), (1, 1), (3, 2), (4, 4), (5, 5), (7, 7), (8, 8), (9, 9), (13, 14), (15, 16)):
        assert a[pos] is fa[fpos], (pos, fpos)
    assert a[2] is outs[2] or (a[2].data_ptr() == outs[2].data_ptr() and a[2].shape == outs[2].shape)  # radii
    assert a[16] is outs[3] and a[18] is outs[4] and a[19] is outs[5]
    assert (a[6], a[10], a[11], a[14], a[17], a[20]) == (SCALE_MOD, TANX, TANY, DEG, NUM_RENDERED, s.debug)
    assert a[12].shape == (3, H, W) and a[12].is_contiguous() and torch.equal(a[12], torch.full((3, H, W), color_grad))


KINDS = {"plain": (False, False), "aux": (True, False), "camera": (False, True), "aux+camera": (True, True)}
REACH = {False: ("colour", "none"), True: ("colour", "aux", "invdepth", "alpha", "all", "none")}


def _run_case(monkeypatch, kind, owner_mode, req, colour, cov, split, reach):
    aux, camera = KINDS[kind]
    native = Native(monkeypatch)
    t, sh_split = _tensors(colour, cov, split, req)
    s = _settings(cam_req=(camera,) * 3)
    cams = (s.viewmatrix, s.projmatrix, s.campos)
    slots = [t.get(kw) for kw, _ in SLOTS]
    needs = tuple(x is not None and x.requires_grad for x in slots)

    owner, registered = None, []
    if owner_mode != "none":
        owner = Deferrer(accepts_sh_split=split)
        left_out = ("means2D",) if owner_mode == "deferring" else ("means2D", "opacities")
        registered = [v for k, v in t.items() if k not in left_out]
        for v in registered:
            register_gradient_sink(v, owner)
    try:
        kw = dict(t)
        if sh_split is not None:
            kw["sh_split"] = sh_split
        if aux:
            kw["aux_outputs"] = True
        if camera:
            kw["camera_grads"] = True
        out = GaussianRasterizer(s)(**kw)

        # ---- the forward ----
        assert len(native.calls) == 1
        fwd_name = "rasterize_gaussians_aux" if aux else "rasterize_gaussians"
        _check_forward_call(native.calls[0], fwd_name, s, t, sh_split)
        fwd = (native.calls[0], native.outs)
        assert len(out) == (4 if aux else 2)
        assert torch.equal(out[0], native.outs[1]) and torch.equal(out[1], native.outs[2])
        assert not out[1].requires_grad
        if aux:
            assert torch.equal(out[2], native.outs[6]) and torch.equal(out[3], native.outs[7])
        sinks = [(k, SLOTS[k][1], slots[k], owner) for k in range(8)
                 if needs[k] and any(slots[k] is r for r in registered)]
        if owner is not None:
            assert len(owner.forwards) == (1 if sinks else 0)
            if sinks:
                assert owner.forwards[0][0] is native.outs[3] and owner.forwards[0][1] == P
        differentiable = any(needs) or camera
        assert all(o.requires_grad == differentiable for k, o in enumerate(out) if k != 1)
        if not differentiable:
            return

        # ---- the loss and what the backward must do with it ----
        gc = reach in ("colour", "all")
        gi, ga = aux and reach in ("aux", "invdepth", "all"), aux and reach in ("aux", "alpha", "all")
        loss = (W_COLOR * out[0]).sum() if gc else _Drop.apply(out[0]).sum()
        if gi:
            loss = loss + (W_INV * out[2]).sum()
        if ga:
            loss = loss + (W_ALPHA * out[3]).sum()
        defers = bool(sinks) and all(k == 1 or not needs[k] or any(e[0] == k for e in sinks) for k in range(8))
        refusal = T_CAM_DEFER if camera and defers else T_AUX_DEFER if (gi or ga) and defers else None
        if refusal is not None:
            with pytest.raises(RuntimeError) as e:
                loss.backward()
            assert str(e.value) == refusal
            assert len(native.calls) == 1 and not owner.deferred and not owner.claims
            return
        loss.backward()
        calls = native.calls[1:]
        expect = {}  # input slot -> the constant its .grad holds
        cam_expect = [None, None, None]
        if not (gc or gi or ga):
            assert not calls
        elif defers:
            assert [c[0] for c in calls] == ["backward_render"]
            a, bkw = calls[0][1], calls[0][2]
            fa = fwd[0][1]
            assert not bkw and len(a) == 16
            assert a[0] is s.bg and a[1] is fa[8] and a[2] is fa[9] and a[3] is s.campos
            assert a[6].is_contiguous() and torch.equal(a[6], torch.full((3, H, W), W_COLOR))
            assert a[10] is native.outs[3] and a[12] is native.outs[4] and a[13] is native.outs[5]
            assert (a[4], a[5], a[7], a[8], a[9], a[11], a[14], a[15]) == (
                TANX, TANY, P, DEG, M if colour == "shs" else 0, NUM_RENDERED, needs[1], False)
            assert len(owner.deferred) == 1 and not owner.claims
            inputs, view, ctx_sinks, ctx_needs = owner.deferred[0]
            assert set(inputs) == {"means3D", "sh", "colors", "scales", "rotations", "cov3D", "scale_modifier",
                                   "degree", "debug", "sh_rest"}
            for key, fpos in (("means3D", 1), ("sh", 14), ("colors", 2), ("scales", 4), ("rotations", 5), ("cov3D", 7)):
                assert inputs[key] is fa[fpos], key
            assert (inputs["scale_modifier"], inputs["degree"], inputs["debug"]) == (SCALE_MOD, DEG, False)
            assert inputs["sh_rest"] is fwd[0][2].get("sh_rest")
            assert len(view) == 8 and view[0] is fa[8] and view[1] is fa[9] and view[2] is s.campos
            assert view[3:7] == (TANX, TANY, W, H) and view[7] is native.outs[3]
            assert len(ctx_sinks) == len(sinks)
            for got, want in zip(ctx_sinks, sinks):
                assert got[:2] == want[:2] and got[2] is want[2] and got[3] is want[3]
            assert ctx_needs == needs
            if needs[1]:
                expect[1] = DM2
        else:
            assert [c[0] for c in calls] == ["backward_impl"]
            a, bkw = calls[0][1], calls[0][2]
            _check_backward_args(a, fwd, s, W_COLOR if gc else 0.0)
            assert set(bkw) <= {"want_all", "sinks", "wait_event", "sh_rest", "aux_grads", "camera"}
            assert bkw["want_all"] is False and set(bkw["sinks"]) == set() and bkw["wait_event"] is None
            assert bkw["sh_rest"] is fwd[0][2].get("sh_rest")
            if gi or ga:
                d_inv, d_alpha = bkw["aux_grads"]
                assert (d_inv is not None, d_alpha is not None) == (gi, ga)
                assert d_inv is None or torch.equal(d_inv, torch.full((1, H, W), W_INV))
                assert d_alpha is None or torch.equal(d_alpha, torch.full((1, H, W), W_ALPHA))
            else:  # the plain backward, as it stands
                assert bkw.get("aux_grads") is None
            assert bkw.get("camera") is (True if camera else None)
            if owner is not None:  # an owner that does not take the view is asked for each buffer, in input order
                assert len(owner.claims) == len(sinks) and all(c is e[2] for c, e in zip(owner.claims, sinks))
                assert not owner.deferred
            expect = {k: GRAD[SLOTS[k][1]] for k in range(8) if needs[k]}
            if camera:
                cam_expect = list(CAM)
        for k, x in enumerate(slots):
            if x is None:
                continue
            if k in expect:
                assert x.grad is not None and x.grad.shape == x.shape, SLOTS[k][0]
                assert torch.equal(x.grad, torch.full(x.shape, expect[k])), SLOTS[k][0]
            else:
                assert x.grad is None, SLOTS[k][0]
        for c, want in zip(cams, cam_expect):
            if want is None:
                assert c.grad is None
            else:
                assert c.grad.shape == c.shape and torch.equal(c.grad, torch.full(c.shape, want))
    finally:
        for v in registered:
            unregister_gradient_sink(v)
        assert not dgr._SINKS


@pytest.mark.parametrize("req", ["all", "means3D", "none"])
@pytest.mark.parametrize("owner_mode", ["none", "deferring", "deferring-but-opacities"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_call_sequence_and_gradients(monkeypatch, kind, owner_mode, req):
    aux, camera = KINDS[kind]
    n = 0
    for colour, cov, split, reach in itertools.product(("shs", "colors_precomp"), ("scale-rot", "cov3D_precomp"),
                                                       (False, True), REACH[aux]):
        if split and (colour != "shs" or camera):
            continue  # sh_split replaces shs; camera_grads refuses it (test_refusals_in_the_call)
        _run_case(monkeypatch, kind, owner_mode, req, colour, cov, split, reach)
        n += 1
    assert n == (4 if camera else 6) * len(REACH[aux])


# ------------------------------------------------------------------------------------------
# the camera tensors that require grad
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("cam_req", [(True, False, False), (False, True, False), (False, False, True),
                                     (True, True, False), (False, False, False)])
def test_camera_flag_follows_campos(monkeypatch, cam_req, aux):
    """backward_impl's `camera` is whether dL/dcampos is wanted; a camera tensor that does not require
    grad gets none; with none of them requiring grad the call is the one without camera_grads."""
    native = Native(monkeypatch)
    t, _ = _tensors("shs", "scale-rot", False, "all")
    s = _settings(cam_req=cam_req)
    out = GaussianRasterizer(s)(**t, aux_outputs=aux, camera_grads=True)
    loss = (W_COLOR * out[0]).sum()
    if aux:
        loss = loss + (W_INV * out[2]).sum()
    loss.backward()
    assert [c[0] for c in native.calls] == ["rasterize_gaussians_aux" if aux else "rasterize_gaussians",
                                            "backward_impl"]
    bkw = native.calls[1][2]
    assert bkw.get("camera") is (cam_req[2] if any(cam_req) else None)
    assert (bkw.get("aux_grads") is not None) == aux
    for c, r, want in zip((s.viewmatrix, s.projmatrix, s.campos), cam_req, CAM):
        assert (c.grad is not None) == r
        if r:
            assert c.grad.shape == c.shape and torch.equal(c.grad, torch.full(c.shape, want))
    for kw, name in SLOTS:
        if kw in t:
            assert torch.equal(t[kw].grad, torch.full(t[kw].shape, GRAD[name]))


# ------------------------------------------------------------------------------------------
# prepared views and bounded forwards (plain calls only)
# ------------------------------------------------------------------------------------------
def _prepared(s, t, triple):
    return dgr.PreparedView(triple, s, (t["means3D"], t.get("shs"), t.get("colors_precomp"), t["opacities"],
                                        t.get("scales"), t.get("rotations"), t.get("cov3D_precomp")))


def test_prepared_view_reaches_the_native_call(monkeypatch):
    native = Native(monkeypatch)
    t, _ = _tensors("shs", "scale-rot", False, "all")
    s = _settings()
    triple = (NUM_RENDERED, torch.ones((P,), dtype=torch.int32), torch.zeros((8,), dtype=torch.uint8), False)
    pv = _prepared(s, t, triple)
    out = GaussianRasterizer(s)(**t, prepared=pv)
    assert len(native.calls) == 1
    _check_forward_call(native.calls[0], "rasterize_gaussians", s, t, None, prepared=triple)
    assert pv.triple is None  # used once
    (W_COLOR * out[0]).sum().backward()
    assert [c[0] for c in native.calls] == ["rasterize_gaussians", "backward_impl"]
    _check_backward_args(native.calls[1][1], (native.calls[0], native.outs), s, W_COLOR)
    with pytest.raises(RuntimeError) as e:
        GaussianRasterizer(s)(**t, prepared=pv)
    assert str(e.value) == "prepare_views: a prepared view is used once"


@pytest.mark.parametrize("split", [False, True])
def test_bounded_forward_passes_the_capacity(monkeypatch, split):
    native = Native(monkeypatch)
    t, sh_split = _tensors("shs", "scale-rot", split, "all")
    s = _settings()
    out = GaussianRasterizer(s)(**t, sh_split=sh_split, binning_capacity=4096)
    _check_forward_call(native.calls[0], "rasterize_gaussians", s, t, sh_split, capacity=4096)
    (W_COLOR * out[0]).sum().backward()
    assert [c[0] for c in native.calls] == ["rasterize_gaussians", "backward_impl"]
    assert native.calls[1][2]["sh_rest"] is native.calls[0][2]["sh_rest"]


# ------------------------------------------------------------------------------------------
# refusals: exception type and full text
# ------------------------------------------------------------------------------------------
def test_refusals_in_the_call(monkeypatch):
    native = Native(monkeypatch)
    t, sh_split = _tensors("shs", "scale-rot", True, "all")
    s = _settings()
    cam_s = _settings(cam_req=(True, True, True))
    r, cam_r = GaussianRasterizer(s), GaussianRasterizer(cam_s)
    pv = object()

    def refused(text, rast=r, exc=RuntimeError, **kw):
        args = dict(t)
        args.update(kw)
        with pytest.raises(exc) as e:
            rast(**{k: v for k, v in args.items() if v is not None})
        assert type(e.value) is exc and str(e.value) == text

    refused(T_SPLIT_PREPARED, sh_split=sh_split, prepared=pv)
    wrong = torch.zeros((P, M - 1, 3), requires_grad=True)
    refused(T_CARRIER, shs=wrong, sh_split=sh_split)
    refused(T_CARRIER, shs=wrong, sh_split=sh_split, aux_outputs=True)
    refused(T_CARRIER, shs=wrong, sh_split=sh_split, binning_capacity=64)
    refused(T_CAP_PREPARED, prepared=pv, binning_capacity=64)
    refused(T_AUX_PREPARED, aux_outputs=True, prepared=pv)
    refused(T_AUX_BOUNDED, aux_outputs=True, binning_capacity=64)
    for aux in (False, True):
        for rast in (r, cam_r):  # refused whether or not a camera tensor requires grad
            refused("camera_grads: not supported with prepared=", rast, camera_grads=True, aux_outputs=aux, prepared=pv)
            refused("camera_grads: not supported with binning_capacity=", rast, camera_grads=True, aux_outputs=aux,
                    binning_capacity=64)
            refused("camera_grads: not supported with sh_split=", rast, camera_grads=True, aux_outputs=aux,
                    sh_split=sh_split)
    # camera_grads' own refusals come first
    refused("camera_grads: not supported with prepared=", camera_grads=True, aux_outputs=True, prepared=pv,
            binning_capacity=64, sh_split=sh_split)
    col = torch.rand((P, 3))
    refused(T_COLOUR, exc=Exception, colors_precomp=col)
    refused(T_COLOUR, exc=Exception, shs=None)
    cov = torch.rand((P, 6))
    refused(T_COV, exc=Exception, cov3D_precomp=cov)
    refused(T_COV, exc=Exception, scales=None, rotations=None)
    refused(T_COV, exc=Exception, scales=None)
    refused(T_COV, exc=Exception, rotations=None, cov3D_precomp=cov)
    assert not native.calls


@pytest.mark.parametrize("aux", [False, True])
def test_sh_split_row_modified_before_the_backward(monkeypatch, aux):
    for which in (0, 1):
        native = Native(monkeypatch)
        t, sh_split = _tensors("shs", "scale-rot", True, "all")
        out = GaussianRasterizer(_settings())(**t, sh_split=sh_split, aux_outputs=aux)
        sh_split[which].add_(1.0)
        loss = (W_COLOR * out[0]).sum() + ((W_INV * out[2]).sum() if aux else 0.0)
        with pytest.raises(RuntimeError) as e:
            loss.backward()
        if which == 1:
            assert str(e.value) == T_SPLIT_MODIFIED
        else:  # features_dc is a saved tensor: autograd's own check comes first, in torch's words
            assert "modified by an inplace operation" in str(e.value) and "[5, 1, 3]" in str(e.value)
        assert len(native.calls) == 1


def test_sh_split_with_a_deferring_owner_that_does_not_accept_it(monkeypatch):
    native = Native(monkeypatch)
    t, sh_split = _tensors("shs", "scale-rot", True, "all")
    owner = Deferrer(accepts_sh_split=False)
    registered = [v for k, v in t.items() if k != "means2D"]
    for v in registered:
        register_gradient_sink(v, owner)
    try:
        out = GaussianRasterizer(_settings())(**t, sh_split=sh_split)
        with pytest.raises(RuntimeError) as e:
            (W_COLOR * out[0]).sum().backward()
        assert str(e.value) == T_SPLIT_DEFER
        assert len(native.calls) == 1 and not owner.deferred
    finally:
        for v in registered:
            unregister_gradient_sink(v)


def test_two_owners_are_each_told_of_the_forward_once(monkeypatch):
    """forwarded() once per distinct owner; the first sink's owner decides the deferral."""
    native = Native(monkeypatch)
    t, _ = _tensors("shs", "scale-rot", False, "all")
    a, b = Deferrer(), Deferrer()
    owners = dict(means3D=a, shs=a, opacities=b, scales=b, rotations=a)
    for k, o in owners.items():
        register_gradient_sink(t[k], o)
    try:
        out = GaussianRasterizer(_settings())(**t)
        assert len(a.forwards) == 1 and len(b.forwards) == 1
        assert a.forwards[0][0] is native.outs[3] and b.forwards[0][0] is native.outs[3]
        (W_COLOR * out[0]).sum().backward()
        assert [c[0] for c in native.calls] == ["rasterize_gaussians", "backward_impl"]  # a does not hold them all
        assert [id(x) for x in a.claims] == [id(t[k]) for k in ("means3D", "shs", "rotations")]
        assert [id(x) for x in b.claims] == [id(t[k]) for k in ("opacities", "scales")]
        assert not a.deferred and not b.deferred
    finally:
        for k in owners:
            unregister_gradient_sink(t[k])


# ------------------------------------------------------------------------------------------
# settings.debug: the snapshot of a failing native call
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("phase", ["forward", "backward"])
def test_debug_snapshot(monkeypatch, tmp_path, capsys, kind, phase):
    aux, camera = KINDS[kind]
    monkeypatch.chdir(tmp_path)
    fwd_name = "rasterize_gaussians_aux" if aux else "rasterize_gaussians"
    native = Native(monkeypatch, fail=fwd_name if phase == "forward" else "backward_impl")
    t, _ = _tensors("shs", "scale-rot", False, "all")
    s = _settings(cam_req=(camera,) * 3, debug=True)
    dump = "snapshot_fw.dump" if phase == "forward" else "snapshot_bw.dump"

    def run():
        out = GaussianRasterizer(s)(**t, aux_outputs=aux, camera_grads=camera)
        assert not list(tmp_path.iterdir())
        ((W_COLOR * out[0]).sum() + ((W_INV * out[2]).sum() if aux else 0.0)).backward()

    with pytest.raises(RuntimeError) as e:
        run()
    assert str(e.value) == f"boom in {native.fail}"
    assert [p.name for p in tmp_path.iterdir()] == [dump]
    assert capsys.readouterr().out == f"\nAn error occured in {phase}. Please forward {dump} for debugging.\n"
    saved = torch.load(tmp_path / dump, weights_only=False)
    call = native.calls[-1][1]
    assert isinstance(saved, tuple) and len(saved) == len(call) == (19 if phase == "forward" else 21)
    for got, want in zip(saved, call):
        assert torch.equal(got, want) if isinstance(want, torch.Tensor) else got == want


def test_no_snapshot_without_debug_or_on_the_prepared_path(monkeypatch, tmp_path, capsys):
    monkeypatch.chdir(tmp_path)
    t, _ = _tensors("shs", "scale-rot", False, "all")
    Native(monkeypatch, fail="rasterize_gaussians")
    with pytest.raises(RuntimeError, match="boom"):
        GaussianRasterizer(_settings(debug=False))(**t)
    s = _settings(debug=True)
    pv = _prepared(s, t, (NUM_RENDERED, torch.ones((P,), dtype=torch.int32), torch.zeros((8,), dtype=torch.uint8),
                          False))
    with pytest.raises(RuntimeError, match="boom"):
        GaussianRasterizer(s)(**t, prepared=pv)
    assert not list(tmp_path.iterdir()) and capsys.readouterr().out == ""


def test_the_constants_differ():
    assert len(set(GRAD.values()) | set(CAM) | {DM2}) == len(GRAD) + 4 and math.isfinite(DM2)
