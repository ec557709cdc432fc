"""Antialiasing (GaussianRasterizer(...)(..., antialiasing=True)) without a GPU: the backward's closed
form against autograd, the autograd layer over recording fakes of the native calls (the manner of
tests/test_autograd_contract_cpu.py, whose fakes and fixtures are reused), and the validation order
of the three new C entries (the tables of tests/test_api_contract_cpu.py and tests/test_camera_cpu.py,
run through the entries they extend and through the new ones)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import dense_ref_aa
import diff_gaussian_rasterization as dgr
import test_api_contract_cpu as api
import test_autograd_contract_cpu as ac
import test_camera_cpu as camt
from diff_gaussian_rasterization import GaussianRasterizer, _native, register_gradient_sink, unregister_gradient_sink

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the closed form against autograd, fp64 ----
def _raw_cases():
    g = torch.Generator().manual_seed(3)
    n = 64
    # random positive-definite raw covariances over six decades of size, plus the named cases:
    # r far below the floor (s held at 0.005: no chain gradient), r just on either side of it, r = 0.54
    L = torch.randn((n, 2, 2), generator=g, dtype=torch.float64) * (10.0 ** torch.empty(n, dtype=torch.float64).uniform_(
        -3, 1.5, generator=g))[:, None, None]
    S = L @ L.transpose(1, 2)
    c00, c01, c11 = S[:, 0, 0], S[:, 0, 1], S[:, 1, 1]
    v54 = 0.3 * (0.54 ** 0.5) / (1 - 0.54 ** 0.5)  # isotropic v with (v / (v + 0.3))^2 = 0.54
    named = torch.tensor([[1e-6, 0.0, 1e-6], [0.0015, 0.0, 0.0015], [0.00152, 0.0, 0.00152], [v54, 0.0, v54],
                          [2e-5, 1e-5, 3e-5]], dtype=torch.float64)
    return (torch.cat([c00, named[:, 0]]), torch.cat([c01, named[:, 1]]), torch.cat([c11, named[:, 2]]), n)


def test_closed_form_matches_autograd_fp64():
    c00, c01, c11, n = _raw_cases()
    g = torch.Generator().manual_seed(4)
    op = torch.rand(c00.shape, generator=g, dtype=torch.float64)
    gout = torch.randn(c00.shape, generator=g, dtype=torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in (op, c00, c01, c11)]
    s, r = dense_ref_aa.scale_of(*leaves[1:])
    (leaves[0] * s * gout).sum().backward()
    # the named cases are what they are meant to be
    assert r[n] < 2.5e-5 / 10 and s[n] == 0.005 and r[n + 1] < 2.5e-5 < r[n + 2]
    assert abs(float(r[n + 3].detach()) - 0.54) < 1e-12
    assert ((r > 2.5e-5) & (r < 0.999)).sum() > n // 2
    got = dense_ref_aa.aa_closed_form(op, gout, c00, c01, c11)
    for k, (a, b) in enumerate(zip(got, leaves)):
        ref = b.grad
        assert torch.all((a - ref).abs() <= 1e-13 * ref.abs().max() + 4e-16 * ref.abs()), (k, (a - ref).abs().max())
    # below the floor the scale is a constant: no gradient reaches the covariance
    for k in (n, n + 1):
        assert all(float(leaves[j].grad[k]) == 0.0 and float(got[j][k]) == 0.0 for j in (1, 2, 3))
    assert float(leaves[1].grad[n + 3]) != 0.0


def test_aa_scale_follows_prep_and_reaches_the_view_matrix():
    """aa_scale's raw covariance + 0.3 is dense_ref._prep's conic, and `view` can be a leaf."""
    import math

    import dense_ref
    import gs_scenes

    W, H = 96, 64
    cam = gs_scenes.look_at_camera((0.4, -0.3, -1.0), (0.1, 0.0, 5.0), W, H)
    d = gs_scenes.random_gaussians(50, 0, cam=gs_scenes.identity_camera(W, H), seed=5)
    f = torch.float64
    view = cam.world_view_transform.to(f).clone().requires_grad_(True)
    tx, ty = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    m3 = d.means3D.to(f)
    c00, c01, c11 = dense_ref_aa.raw_cov2d(m3, view, tx, ty, W, H, scales=d.scales.to(f), rots=d.rotations.to(f))
    q = dense_ref._prep(m3, torch.zeros_like(m3), d.opacities.to(f), view, cam.full_proj_transform.to(f),
                        cam.camera_center.to(f), tx, ty, W, H, shs=d.shs.to(f), deg=0, scales=d.scales.to(f),
                        rots=d.rotations.to(f))
    a, b, c = c00 + 0.3, c01, c11 + 0.3
    det = a * c - b * b
    assert torch.allclose(torch.stack([c / det, -b / det, a / det], -1), q["conic"], rtol=1e-12, atol=0)
    s = dense_ref_aa.aa_scale(m3, view, tx, ty, W, H, scales=d.scales.to(f), rots=d.rotations.to(f))
    assert s.dtype == f and bool(((s >= 0.005) & (s < 1)).all())
    s.sum().backward()
    assert view.grad is not None and float(view.grad.abs().max()) > 0


# ---- the public argument, the header, the symbols ----
def test_forward_has_antialiasing_as_its_last_keyword():
    p = inspect.signature(GaussianRasterizer.forward).parameters
    assert list(p)[-1] == "antialiasing" and p["antialiasing"].default is False
    assert len(dgr.GaussianRasterizationSettings._fields) == 12


def test_header_defines_has_antialiasing_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    assert re.search(r"^#define GSRAST_HAS_ANTIALIASING 1$", text, re.M)
    assert int(re.search(r"#define GSRAST_ABI_VERSION (\d+)", text).group(1)) == 17 == _native.load().gs_abi_version()
    for name in ("gs_forward_preprocess_aa", "gs_backward_accumulate_aa", "gs_backward_camera_aa"):
        assert re.search(r"\bint %s\(" % name, text) and hasattr(_native.load(), name)
        ext = {"gs_forward_preprocess_aa": "gs_forward_preprocess", "gs_backward_accumulate_aa":
               "gs_backward_accumulate_aux", "gs_backward_camera_aa": "gs_backward_camera"}[name]
        assert _native.SIGNATURES[name][1] == _native.SIGNATURES[ext][1] + [ctypes.c_int]


# ---- the autograd layer over fakes ----
T_AA = "antialiasing: not supported with %s="
T_AA_DEFER = ("antialiasing: not supported with a deferring gradient owner (GradBucket(defer=True), the fused "
              "backward + Adam of gs_train_step)")


class Native(ac.Native):
    """ac.Native plus the antialiased forward."""

    def __init__(self, monkeypatch, fail=None):
        super().__init__(monkeypatch, fail)
        monkeypatch.setattr(dgr._C, "rasterize_gaussians_aa", self.rasterize_gaussians_aa)

    def rasterize_gaussians_aa(self, *a, **kw):
        out = self._forward("rasterize_gaussians_aa", a, kw)
        if kw.get("aux"):
            self.outs = out + (torch.rand((1, a[12], a[13])), torch.rand((1, a[12], a[13])))
        return self.outs


@pytest.mark.parametrize("kind", list(ac.KINDS))
@pytest.mark.parametrize("colour,cov", [("shs", "scale-rot"), ("colors", "cov3D")])
def test_flag_reaches_the_forward_and_backward_calls(monkeypatch, kind, colour, cov):
    aux, camera = ac.KINDS[kind]
    native = Native(monkeypatch)
    t, _ = ac._tensors(colour, cov, False, "all")
    s = ac._settings(cam_req=(camera,) * 3)
    out = GaussianRasterizer(s)(**t, aux_outputs=aux, camera_grads=camera, antialiasing=True)
    assert [c[0] for c in native.calls] == ["rasterize_gaussians_aa"]
    _n, a, kw = native.calls[0]
    assert kw == {"aux": aux} and len(a) == 19  # rasterize_gaussians' nineteen arguments
    ac._check_forward_call(("x", a, {}), "x", s, t, None)
    assert len(out) == (4 if aux else 2)
    loss = (ac.W_COLOR * out[0]).sum()
    if aux:
        loss = loss + (ac.W_INV * out[2]).sum() + (ac.W_ALPHA * out[3]).sum()
    loss.backward()
    assert [c[0] for c in native.calls[1:]] == ["backward_impl"]
    _n, a, kw = native.calls[1]
    ac._check_backward_args(a, (native.calls[0], native.outs), s, ac.W_COLOR)
    assert set(kw) == {"want_all", "sinks", "wait_event", "sh_rest", "aux_grads", "camera", "aa_opacity"}
    assert kw["aa_opacity"].data_ptr() == t["opacities"].data_ptr() and kw["aa_opacity"].shape == (ac.P, 1)
    assert kw["sh_rest"] is None and kw["want_all"] is False
    assert (kw["aux_grads"] is not None) == aux and kw["camera"] is (True if camera else None)
    for key, name in ac.SLOTS:
        if key in t:
            assert torch.equal(t[key].grad, torch.full(ac.GRAD_SHAPE[name], ac.GRAD[name])), key
    if camera:
        assert torch.equal(s.viewmatrix.grad, torch.full((4, 4), ac.CAM[0]))
        assert torch.equal(s.campos.grad, torch.full((3,), ac.CAM[2]))


@pytest.mark.parametrize("kind", list(ac.KINDS))
@pytest.mark.parametrize("how", ["absent", "false"])
def test_without_the_keyword_the_native_calls_are_todays(monkeypatch, kind, how):
    """Neither a call without the keyword nor antialiasing=False makes a new call or passes a new
    argument: the recorded sequence is the one tests/test_autograd_contract_cpu.py pins."""
    aux, camera = ac.KINDS[kind]
    native = Native(monkeypatch)
    t, _ = ac._tensors("shs", "scale-rot", False, "all")
    s = ac._settings(cam_req=(camera,) * 3)
    extra = {} if how == "absent" else {"antialiasing": False}
    out = GaussianRasterizer(s)(**t, aux_outputs=aux, camera_grads=camera, **extra)
    fwd_name = "rasterize_gaussians_aux" if aux else "rasterize_gaussians"
    assert [c[0] for c in native.calls] == [fwd_name]
    ac._check_forward_call(native.calls[0], fwd_name, s, t, None)
    (ac.W_COLOR * out[0]).sum().backward()
    assert [c[0] for c in native.calls[1:]] == ["backward_impl"]
    _n, a, kw = native.calls[1]
    assert len(a) == 21 and "aa_opacity" not in kw
    assert set(kw) <= {"want_all", "sinks", "wait_event", "sh_rest", "aux_grads", "camera"}


@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("name", ["prepared", "binning_capacity", "sh_split"])
def test_forward_refusals(monkeypatch, name, aux):
    native = Native(monkeypatch)
    t, sh_split = ac._tensors("shs", "scale-rot", True, "all")
    s = ac._settings()
    value = {"prepared": object(), "binning_capacity": 1000, "sh_split": sh_split}[name]
    with pytest.raises(RuntimeError) as e:
        GaussianRasterizer(s)(**t, aux_outputs=aux, antialiasing=True, **{name: value})
    assert str(e.value) == T_AA % name and not native.calls
    # and below the module: the Function's own check, and the ctypes layer's
    with pytest.raises(RuntimeError) as e:
        dgr.rasterize_gaussians(t["means3D"], t["means2D"], t["shs"], torch.Tensor([]), t["opacities"], t["scales"],
                                t["rotations"], torch.Tensor([]), s, antialiasing=True, **{name: value})
    assert str(e.value) == T_AA % name and not native.calls


def test_ctypes_layer_refusals():
    """_C refuses the same combinations before it looks at a tensor's device."""
    x = object()
    for kw, name in ((dict(prepared=(1, 2, 3)), "prepared"), (dict(capacity=10), "binning_capacity")):
        with pytest.raises(RuntimeError) as e:
            dgr._C._forward_ctypes(x, 4, 4, 0, 1.0, 0.5, 0.5, False, False, antialiasing=True, **kw)
        assert str(e.value) == T_AA % name
    m = torch.zeros((2, 3))
    with pytest.raises(RuntimeError) as e:
        dgr._C.backward_impl(None, m, None, None, None, None, 1.0, None, None, None, 0.5, 0.5, None, None, 0, None,
                             None, 0, None, None, False, sh_rest=m, aa_opacity=torch.ones((2, 1)))
    assert str(e.value) == T_AA % "sh_split"


@pytest.mark.parametrize("aux", [False, True])
def test_deferring_owner_is_refused_in_the_backward(monkeypatch, aux):
    native = Native(monkeypatch)
    t, _ = ac._tensors("shs", "scale-rot", False, "all")
    s = ac._settings()
    owner = ac.Deferrer()
    owner.accepts_aux = True
    registered = [v for k, v in t.items() if k != "means2D"]
    for v in registered:
        register_gradient_sink(v, owner)
    try:
        out = GaussianRasterizer(s)(**t, aux_outputs=aux, antialiasing=True)
        with pytest.raises(RuntimeError) as e:
            (out[0].sum() + (out[3].sum() if aux else 0)).backward()
        assert str(e.value) == T_AA_DEFER
        assert len(native.calls) == 1 and not owner.deferred and not owner.claims
    finally:
        for v in registered:
            unregister_gradient_sink(v)


def test_debug_snapshots_include_the_flag(monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    t, _ = ac._tensors("shs", "scale-rot", False, "all")
    s = ac._settings(debug=True)
    Native(monkeypatch, fail="rasterize_gaussians_aa")
    with pytest.raises(RuntimeError, match="boom"):
        GaussianRasterizer(s)(**t, antialiasing=True)
    snap = torch.load(tmp_path / "snapshot_fw.dump", weights_only=False)
    assert len(snap) == 20 and snap[-1] is True and torch.equal(snap[3], t["opacities"].detach())
    Native(monkeypatch, fail="backward_impl")
    out = GaussianRasterizer(s)(**t, antialiasing=True)
    with pytest.raises(RuntimeError, match="boom"):
        out[0].sum().backward()
    snap = torch.load(tmp_path / "snapshot_bw.dump", weights_only=False)
    assert len(snap) == 23 and snap[-2] is True and torch.equal(snap[-1], t["opacities"].detach())


# ---- the validation order of the three entries ----
X = api.X
E_AA_SPLIT = "antialiasing: not supported with split SH rows (shs_rest)"
PARAMS = {
    "gs_forward_preprocess_aa": api.PARAMS["gs_forward_preprocess"] + " antialiasing",
    "gs_backward_accumulate_aa": api.PARAMS["gs_backward_accumulate_aux"] + " antialiasing",
}


def _call(entry, over, aa):
    """api.call for the new entries (same defaults), the flag last."""
    names = PARAMS[entry].split()
    assert not set(over) - set(names)
    nr = ctypes.c_longlong(api.SENTINEL)
    args, left = [], None
    for n in names:
        if n == "antialiasing":
            args.append(aa)
        elif n == "nr":
            v = over.get("nr", nr)
            args.append(None if v is None else ctypes.byref(nr))
            left = None if v is None else nr
        elif n == "shs_rest" and n not in over:
            args.append(None)
        else:
            args.append(over[n] if n in over else api._default(n))
    lib = _native.load()
    rc = getattr(lib, entry)(*args)
    return rc, lib.gs_last_error().decode(), None if left is None else left.value


def _rows():
    rows = []
    e, x = "gs_forward_preprocess_aa", "gs_forward_preprocess"
    for r in api.front_rows(x, 0, api.E_OUT) + api.colour_rows(x, 0, api.E_OUT) + [
            (x, dict(nr=None), 1, api.E_OUT, None), (x, dict(nr=None, W=0), 1, api.E_SIZE % (0, 16), None)]:
        rows += [(e, x, r[1], aa, r[2:]) for aa in (0, 1)]  # the flag changes no check of the forward
    e, x = "gs_backward_accumulate_aa", "gs_backward_accumulate_aux"
    base = (api.backward_rows(x) + api.colour_rows(x, None, api.E_BUF) + api.split3_rows(x, None)
            + [(x, dict(dL_dout_invdepth=None, dL_dout_alpha=None, geom=None), 1, api.E_BUF, None)])
    for r in base:
        rows.append((e, x, r[1], 0, r[2:]))
        want = r[2:]
        if "shs_rest" in r[1]:  # refused in front of every other check
            want = (1, E_AA_SPLIT, None)
        elif r[1].get("opac", X) is None and r[3] == api.E_BUF:  # the antialiased backward reads the opacities
            want = (1, api.E_IN, None)
        rows.append((e, x, r[1], 1, want))
    rows += [(e, x, dict(shs_rest=X, P=-1), 1, (1, E_AA_SPLIT, None)),
             (e, x, dict(opac=None, P=0), 1, (0, "", None)),
             (e, x, dict(opac=None, W=0), 1, (1, api.E_SIZE % (0, 16), None)),
             (e, x, dict(opac=None, means3D=None, cov3D=X), 1, (1, api.E_IN, None))]
    return rows


ROWS = _rows()


@pytest.mark.parametrize("row", ROWS, ids=[f"{i:03d}-{r[0][3:]}-aa{r[3]}[" + ",".join(r[2]) + "]"
                                           for i, r in enumerate(ROWS)])
def test_new_entries_early_return(row):
    entry, extended, over, aa, want = row
    assert _call(entry, over, aa) == tuple(want), (entry, over, aa)
    if aa == 0:  # the entry it extends says the same
        assert api.call(extended, over) == tuple(want)


def test_new_entry_tables_match_the_declared_signatures():
    for entry, names in PARAMS.items():
        assert len(names.split()) == len(_native.SIGNATURES[entry][1]), entry
    assert len(camt.PARAMS) + 1 == len(_native.SIGNATURES["gs_backward_camera_aa"][1])
    assert {r[3] for r in ROWS} == {0, 1}


CAM_ROWS = [(over, text, aa) for over, text in camt.ROWS for aa in (0, 1)]


@pytest.mark.parametrize("over,text,aa", CAM_ROWS,
                         ids=[f"{i:02d}-aa{r[2]}-" + ",".join(r[0]) for i, r in enumerate(CAM_ROWS)])
def test_backward_camera_aa_early_return(over, text, aa):
    lib = _native.load()
    args = [over[n] if n in over else camt.DEFAULTS.get(n, camt.X) for n in camt.PARAMS]
    if aa and over.get("opac", camt.X) is None and text == camt.E_BUF:
        text = camt.E_IN  # the antialiased camera gradient reads the opacities
    assert lib.gs_backward_camera_aa(*args, aa) == 1
    assert lib.gs_last_error().decode() == text
    if aa == 0:
        assert lib.gs_backward_camera(*args) == 1 and lib.gs_last_error().decode() == text
