"""The K-view per-Gaussian backward (k_backward_gaussians behind gs_backward_gaussians /
gs_backward_gaussians_range) at its row, view and layout edges, on the constructed scenes of
tests/fused_views_cases.py.

Harness: per view `_C.rasterize_gaussians` then `_C.backward_render` (the view's record sums stay in its
geomBuffer), then `_C.backward_gaussians(..., views, outs, accumulate, first=, count=)`.

Reference A (bitwise): every view's gradients from the single-view `_C.rasterize_gaussians_backward` on a
fresh forward of its own, combined in fp32 as `g = g0; g += g1; ...` in view order, starting from the
prefilled buffer where the output's GS_ACC bit is set.  Everything bitwise is compared with torch.equal
on the int32 view of the tensors (a NaN payload compares, -0 differs from +0).

Reference B (fp64): tests/dense_ref.py per view under autograd, with tests/test_gpu_dense.py's rules:
its RTOL, its 5e-5 of max for the covariance chain, its masking of the pixels flagged near a decision
(at most 2 % per view), its 4x-of-dense-fp32 conditioning check.  The bound of a K-view sum is the sum of
the per-view bounds RTOL |ref_v| + frac max|ref_v|.

The host path is the one `_C` selects (the torch extension when it is loaded) and, for the cases that
turn on host arithmetic (ranges, view counts, misaligned bases), the ctypes path as well.
"""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import dense_ref
import fused_views_cases as fvc
import gs_scenes
from gpu_checks import RTOL
from test_gpu_dense import CHAIN

pytestmark = pytest.mark.gpu

CHAIN_FRAC = 5e-5  # test_gpu_dense._run_and_compare's default chain_frac
NAMES = ("colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations")
PAYLOAD = 0x7FC0BEEF  # a quiet NaN with a recognisable mantissa
ALL = 0xFF
RANGES = ((0, 600), (0, 1), (599, 1), (1, 255), (1, 256), (255, 2), (256, 256), (257, 343), (3, 597), (300, 0))
RANGE_LAYOUTS = {"sh3_m16": (3, 16, "sh"), "sh2_m9": (2, 9, "sh"), "sh1_m4": (1, 4, "sh"), "colors": (0, 1, "colors")}


def _C():
    from diff_gaussian_rasterization import _C as c

    return c


@pytest.fixture(params=["selected", "ctypes"])
def host_path(request, monkeypatch):
    """The host path `_C` selects, and the ctypes one (the same when the extension is not loaded)."""
    if request.param == "ctypes":
        monkeypatch.setattr(_C(), "_EXT", None)
    return request.param


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _payload(shape, device):
    return torch.full(shape, PAYLOAD, dtype=torch.int32, device=device).view(torch.float32)


class Case:
    """One scene on the device with its K views prepared for backward_gaussians, and every view's
    single-view gradients (reference A's pieces).  Built once per key and never modified."""

    def __init__(self, leaves, cams, D, device, mod=1.0, seed=100, masks=None):
        c = _C()
        self.L = {k: v.to(device).contiguous() for k, v in leaves.items()}
        self.cams, self.D, self.mod, self.device = list(cams), D, mod, device
        self.P = self.L["means3D"].shape[0]
        self.M = self.L["shs"].shape[1] if "shs" in self.L else 0
        self.dpix = [gs_scenes.dl_dimage(cam.image_height, cam.image_width, seed=seed + v, scale=1.0).to(device)
                     for v, cam in enumerate(cams)]
        if masks is not None:  # reference B: dL/dpix zeroed at the flagged pixels
            self.dpix = [d * m.to(device)[None] for d, m in zip(self.dpix, masks)]
        self.shapes = dict(colors=(self.P, 3), opacity=(self.P, 1), means3D=(self.P, 3), cov3D=(self.P, 6),
                           sh=(self.P, self.M, 3), scales=(self.P, 3), rotations=(self.P, 4))
        self.names = tuple(n for n in NAMES if not (n == "sh" and "shs" not in self.L)
                           and not (n in ("scales", "rotations") and "cov3D" in self.L))
        self.views, self.radii, self.per_view = [], [], []
        for cam, dp in zip(self.cams, self.dpix):
            s, (num, _, radii, geom, binb, imgb) = self._forward(cam)
            c.backward_render(s.bg, s.viewmatrix, s.projmatrix, s.campos, s.tanfovx, s.tanfovy, dp, self.P, D, self.M,
                              geom, num, binb, imgb, False, False)
            self.views.append((s.viewmatrix, s.projmatrix, s.campos, s.tanfovx, s.tanfovy, cam.image_width,
                               cam.image_height, geom))
            self.radii.append(radii)
            # the single-view backward on a forward state of its own
            s, (num, _, radii1, geom1, binb, imgb) = self._forward(cam)
            E = torch.Tensor([])
            L = self.L
            out = c.rasterize_gaussians_backward(
                s.bg, L["means3D"], radii1, L.get("colors", E), L.get("scales", E), L.get("rotations", E), mod,
                L.get("cov3D", E), s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, dp, L.get("shs", E), D, s.campos,
                geom1, num, binb, imgb, False)
            assert torch.equal(radii, radii1)
            self.per_view.append({n: t.reshape(self.shapes[n]) for n, t in zip(NAMES, out[1:]) if n in self.names})
        torch.cuda.synchronize()

    def _forward(self, cam):
        s = gs_scenes.raster_settings_for(cam, self.D, scale_modifier=self.mod, device=self.device)
        E, L = torch.Tensor([]), self.L
        return s, _C().rasterize_gaussians(
            s.bg, L["means3D"], L.get("colors", E), L["opacities"], L.get("scales", E), L.get("rotations", E), self.mod,
            L.get("cov3D", E), s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, cam.image_height, cam.image_width,
            L.get("shs", E), self.D, s.campos, False, False)

    def prefill(self, kind, names=None, seed=7):
        """Output buffers: "payload" (NaNs that a write must replace) or "random" (what an accumulating call adds to)."""
        g = torch.Generator(device=self.device).manual_seed(seed)
        every = {n: (_payload(self.shapes[n], self.device) if kind == "payload"
                     else torch.randn(self.shapes[n], device=self.device, generator=g))
                 for n in self.names}  # (the same values whichever names are asked for)
        return {n: every[n] for n in (names or self.names)}

    def fused(self, outs, acc, first=0, count=None, order=None, L=None):
        L = L or self.L
        views = self.views if order is None else [self.views[v] for v in order]
        _C().backward_gaussians(L["means3D"], L.get("shs"), L.get("colors"), L.get("scales"), L.get("rotations"),
                                L.get("cov3D"), self.mod, self.D, views, outs, acc, first=first, count=count)
        return outs

    def ref_a(self, pre, acc, order=None, names=None):
        """g = g0 (or the prefill, with the output's bit); g += g_v in view order."""
        C = _C()
        out = {}
        for n in (names or self.names):
            g = pre[n].clone() if acc & C.GS_ACC[n] else None
            for v in (range(len(self.views)) if order is None else order):
                g = self.per_view[v][n].clone() if g is None else g.add_(self.per_view[v][n])
            out[n] = g
        return out

    def check_a(self, acc, kind=None, order=None, names=None, what=()):
        """One whole fused call against reference A; returns its outputs."""
        pre = self.prefill(kind or ("random" if acc else "payload"), names)
        got = self.fused({n: t.clone() for n, t in pre.items()}, acc, order=order)
        ref = self.ref_a(pre, acc, order, names)
        for n in ref:
            assert _same(got[n], ref[n]), (*what, n, acc, order, _first_diff(got[n], ref[n]))
        return got


def _first_diff(a, b):
    bad = (a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).reshape(a.shape[0], -1)
    rows = torch.nonzero(bad.any(1)).flatten()
    if rows.numel() == 0:
        return "equal"
    r = int(rows[0])
    return f"{rows.numel()} rows differ, first {r}: {a[r].flatten()[:6].tolist()} != {b[r].flatten()[:6].tolist()}"


_CASES = {}


def _case(key, build):
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


def _layout_case(device, P, D, M, kind, K=3, mod=1.0):
    return _case(("layout", P, D, M, kind, K, mod),
                 lambda: Case(fvc.layout_scene(P, D, M, kind), fvc.ring_cameras(K), D, device, mod=mod))


# ------------------------------------------------------------------------------------------
# 1. ranges
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(RANGE_LAYOUTS))
def test_range_rows_equal_the_whole_call_and_the_rest_is_untouched(device, host_path, layout):
    """P = 600 (blocks of 256 / 256 / 88 rows), K = 3: a call for [first, first + count) writes exactly
    those rows of all the outputs, with the whole call's bits; every other row keeps its NaN payload."""
    D, M, kind = RANGE_LAYOUTS[layout]
    c = _layout_case(device, 600, D, M, kind)
    whole = c.check_a(0)
    for n, t in whole.items():  # the whole call left no payload behind
        assert not (t.view(torch.int32) == PAYLOAD).any(), n
    for first, count in RANGES:
        got = c.fused(c.prefill("payload"), 0, first=first, count=count)
        for n, t in got.items():
            inside = torch.zeros(c.P, dtype=torch.bool, device=device)
            inside[first:first + count] = True
            assert _same(t[inside], whole[n][inside]), (layout, first, count, n, _first_diff(t[inside], whole[n][inside]))
            assert (t[~inside].view(torch.int32) == PAYLOAD).all(), (layout, first, count, n)


@pytest.mark.parametrize("layout", list(RANGE_LAYOUTS))
def test_union_of_chunks_equals_one_whole_call(device, host_path, layout):
    """GradBucket's chunk bounds P * c // chunks for 2, 3 and 7 chunks: written, and with every GS_ACC bit
    over a random prefill."""
    D, M, kind = RANGE_LAYOUTS[layout]
    c = _layout_case(device, 600, D, M, kind)
    for acc in (0, ALL):
        whole = c.check_a(acc)
        for chunks in (2, 3, 7):
            got = c.prefill("random" if acc else "payload")
            bounds = [c.P * k // chunks for k in range(chunks + 1)]
            for lo, hi in zip(bounds, bounds[1:]):
                c.fused(got, acc, first=lo, count=hi - lo)
            for n in got:
                assert _same(got[n], whole[n]), (layout, acc, chunks, n, _first_diff(got[n], whole[n]))


# ------------------------------------------------------------------------------------------
# 2. layouts
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc", [0, ALL], ids=["written", "accumulated"])
@pytest.mark.parametrize("D,M", fvc.LAYOUTS)
def test_every_row_layout(device, D, M, acc):
    """Every (active degree, stored coefficients) pair at P = 257 (one full block and one row): the
    coefficients past (D + 1)^2 are exactly zero when written and exactly kept when accumulated."""
    c = _layout_case(device, 257, D, M, "sh")
    pre = c.prefill("random" if acc else "payload")
    got = c.fused({n: t.clone() for n, t in pre.items()}, acc)
    ref = c.ref_a(pre, acc)
    for n in ref:
        assert _same(got[n], ref[n]), (D, M, acc, n, _first_diff(got[n], ref[n]))
    k = (D + 1) ** 2
    tail = got["sh"][:, k:]
    if acc:
        assert _same(tail, pre["sh"][:, k:])
    else:
        assert (tail.contiguous().view(torch.int32) == 0).all()
    assert (got["sh"][:, :k] != pre["sh"][:, :k]).any()


@pytest.mark.parametrize("acc", [0, ALL], ids=["written", "accumulated"])
def test_precomputed_colours_layout(device, acc):
    c = _layout_case(device, 257, 0, 1, "colors")
    assert "sh" not in c.names
    c.check_a(acc)


@pytest.mark.parametrize("which", ["shs", "sh_out"])
@pytest.mark.parametrize("D,M", [(1, 16), (3, 16), (1, 4)])
def test_base_off_16_bytes(device, host_path, D, M, which):
    """The SH rows, and separately the dL/dsh output, as contiguous slices of a larger buffer starting at
    element 1, 2 and 3 (a view into a flat bucket): bit-identical to the aligned run."""
    c = _layout_case(device, 257, D, M, "sh")
    n = c.P * M * 3
    for acc in (0, ALL):
        want = c.check_a(acc)
        for off in (1, 2, 3):
            pre = c.prefill("random" if acc else "payload")
            L = dict(c.L)
            if which == "shs":
                L["shs"] = torch.zeros(n + 4, device=device)[off:off + n].view(c.P, M, 3).copy_(c.L["shs"])
                assert L["shs"].data_ptr() % 16 == 4 * off and L["shs"].is_contiguous()
            else:
                big = _payload((n + 4,), device)
                sh = big[off:off + n].view(c.P, M, 3).copy_(pre["sh"])
                assert sh.data_ptr() % 16 == 4 * off and sh.is_contiguous()
                pre["sh"] = sh
            got = c.fused(pre, acc, L=L)
            for name in got:
                assert _same(got[name], want[name]), (D, M, which, off, acc, name, _first_diff(got[name], want[name]))
            if which == "sh_out":  # nothing written in front of or behind the slice
                edge = torch.cat([big[:off], big[off + n:]])
                assert (edge.view(torch.int32) == PAYLOAD).all()


# ------------------------------------------------------------------------------------------
# 3. view count
# ------------------------------------------------------------------------------------------
MARKED = 24


def _ring_case(device, K):
    marked = K in (9, 17)

    def build():
        leaves = fvc.layout_scene(300, 3, 16, marked=MARKED)
        return Case(leaves, fvc.ring_cameras(K, last_target=fvc.MARK_TARGET if marked else None), 3, device)

    return _case(("ring", K), build)


@pytest.mark.parametrize("acc", ["none", "all", "sh"])
@pytest.mark.parametrize("K", [1, 2, 8, 9, 16, 17])
def test_view_count(device, host_path, K, acc):
    """1 to 17 views (passes of 8): the caller's GS_ACC bits hold for the first pass only, the later
    passes add.  K = 9 and 17: the last view is the only one that sees the marked Gaussians."""
    c = _ring_case(device, K)
    bits = {"none": 0, "all": ALL, "sh": _C().GS_ACC["sh"]}[acc]
    # mixed: the outputs without their bit are written over a payload
    pre = c.prefill("random")
    if acc != "all":
        pay = c.prefill("payload")
        pre = {n: (pre[n] if bits & _C().GS_ACC[n] else pay[n]) for n in pre}
    got = c.fused({n: t.clone() for n, t in pre.items()}, bits)
    ref = c.ref_a(pre, bits)
    for n in ref:
        assert _same(got[n], ref[n]), (K, acc, n, _first_diff(got[n], ref[n]))
    if K == 1 and not bits:  # the single-view backward itself
        for n in got:
            assert _same(got[n], c.per_view[0][n]), n
    if K in (9, 17):
        seen = torch.stack([r > 0 for r in c.radii], 1)[c.P - MARKED:]
        assert seen[:, -1].all() and not seen[:, :-1].any()
        if not bits:
            for n in got:  # 0 + ... + 0 + g: the last view's own rows (a -0 of its becomes +0 in the sum)
                assert _same(got[n][c.P - MARKED:], c.per_view[-1][n][c.P - MARKED:] + 0.0), n
            assert (got["sh"][c.P - MARKED:] != 0).any() and (got["means3D"][c.P - MARKED:] != 0).any()


# ------------------------------------------------------------------------------------------
# reference B
# ------------------------------------------------------------------------------------------
def _dense_views(leaves, cams, D, mod, dtype, dpix=None):
    """dense_ref.render_local per view on the CPU.  Without dpix: (radii, flag) per view.  With dpix (already
    masked): every view's gradients of sum(img * dpix) by autograd, [view][leaf]."""
    out = []
    for v, cam in enumerate(cams):
        t = {k: x.detach().cpu().to(dtype).clone().requires_grad_(dpix is not None) for k, x in leaves.items()}
        img, radii, flag = dense_ref.render_local(
            t["means3D"], torch.zeros_like(t["means3D"]), t["opacities"], cam.world_view_transform.to(dtype),
            cam.full_proj_transform.to(dtype), cam.camera_center.to(dtype), math.tan(cam.FoVx / 2),
            math.tan(cam.FoVy / 2), cam.image_width, cam.image_height, torch.zeros(3, dtype=dtype), shs=t.get("shs"),
            deg=D, colors=t.get("colors"), scales=t.get("scales"), rots=t.get("rotations"), cov3D=t.get("cov3D"), mod=mod)
        if dpix is None:
            out.append((radii, flag))
            continue
        (img * dpix[v].cpu().to(dtype)).sum().backward()
        out.append({k: (x.grad if x.grad is not None else torch.zeros_like(x)) for k, x in t.items()})
    return out


LEAF_OF = dict(colors="colors", opacity="opacities", means3D="means3D", cov3D="cov3D", sh="shs", scales="scales",
               rotations="rotations")


def _check_b(device, key, leaves, cams, D, mod=1.0):
    """The fused call over all views against the fp64 dense reference, test_gpu_dense's way."""
    pre = _dense_views(leaves, cams, D, mod, torch.float64)
    masks = []
    for v, (radii, flag) in enumerate(pre):
        print(f"[dense] view {v}: flagged pixels {int(flag.sum())}/{flag.numel()}")
        assert float(flag.double().mean()) <= 0.02
        masks.append(~flag)
    c = _case(("B",) + key, lambda: Case(leaves, cams, D, device, mod=mod, masks=masks))
    rdiff = np.zeros(c.P, bool)
    for (radii, _), got in zip(pre, c.radii):
        rdiff |= (radii != got.cpu()).numpy()
    # (a Gaussian whose fp32 radius differed would also need its rectangle masked, as test_gpu_dense does:
    # these scenes have none)
    assert not rdiff.any(), f"{int(rdiff.sum())} radii differ"
    got = c.check_a(0)
    dp = [d.cpu() for d in c.dpix]
    r64 = _dense_views(leaves, cams, D, mod, torch.float64, dp)
    r32 = _dense_views(leaves, cams, D, mod, torch.float32, dp)
    for n in c.names:
        leaf = LEAF_OF[n]
        if leaf not in leaves:  # dL/dcolors of SH inputs, dL/dcov3D of scale / rotation inputs: no leaf (reference A only)
            continue
        g = got[n].double().cpu().numpy().reshape(c.P, -1)
        per = [r[leaf].numpy().reshape(c.P, -1) for r in r64]
        ref = sum(per)
        frac = CHAIN_FRAC if leaf in CHAIN else RTOL
        bound = sum(RTOL * np.abs(p) + frac * np.abs(p).max(initial=0.0) for p in per)
        d = np.abs(g - ref)
        scale = sum(np.abs(p).max(initial=0.0) for p in per)
        print(f"d{leaf}: max|d| {d.max():.3e}  sum of max|ref_v| {scale:.3e}  worst d / bound {(d / bound).max():.3f}")
        assert scale > 0, leaf
        bad = d > bound
        assert not bad.any(), f"d{leaf}: {int(bad.sum())}/{bad.size} beyond tol, max|d| {d.max():.3e}, scale {scale:.3e}"
        if leaf in CHAIN:  # conditioning: within 4x of the dense reference's own fp32 run, summed the same way
            n32 = None
            for r in r32:
                n32 = r[leaf].clone() if n32 is None else n32.add_(r[leaf])
            d_32 = np.abs(n32.double().numpy().reshape(c.P, -1) - ref).max()
            print(f"  d{leaf}: max|hip - f64| {d.max():.3e}  max|dense f32 - f64| {d_32:.3e}")
            assert d.max() <= 4.0 * d_32 + RTOL * scale, (leaf, d.max(), d_32, scale)
    return c


@pytest.mark.parametrize("D,M,kind,mod", [(3, 16, "sh", 1.0), (1, 16, "sh", 1.0), (2, 16, "sh", 1.0), (2, 9, "sh", 0.7),
                                          (0, 1, "colors", 1.0), (1, 4, "cov3d", 1.0)],
                         ids=["staged", "vector_rows", "scalar_padded", "scalar_scale_modifier", "colours", "cov3d"])
def test_layouts_against_the_dense_reference(device, D, M, kind, mod):
    """One case per kernel path (staged rows, 16-byte rows of a lower active degree, scalar rows with and
    without padding, the colours kernel) and input kind, three views of three sizes."""
    P = 160
    _check_b(device, ("layout", P, D, M, kind, mod), fvc.layout_scene(P, D, M, kind), fvc.ring_cameras(3), D, mod)


# ------------------------------------------------------------------------------------------
# 4. visibility
# ------------------------------------------------------------------------------------------
def _vis_case(device, D):
    def build():
        s = fvc.visibility_scene()
        return Case(s.leaves, s.cams, D, device)

    return _case(("vis", D), build)


@pytest.mark.parametrize("D", [3, 1])
def test_visibility_patterns_every_view_order(device, D):
    """Gaussians seen by any subset of the three views (also: not by view 0 and by a later one, by none),
    colour clamps that differ between the views: the kernels see the reference's membership, and each of
    the 6 view orders matches its own reference A, written and accumulated."""
    s = fvc.visibility_scene()
    c = _vis_case(device, D)
    op = s.leaves["opacities"].numpy()
    gpu = np.stack([fvc.contributes(r.cpu().numpy(), op) for r in c.radii], 1)
    ref = np.stack([fvc.contributes(fvc.dense_prep(s.leaves, cam, D)["radii"].numpy(), op) for cam in s.cams], 1)
    assert np.array_equal(gpu, ref) and np.array_equal(gpu, s.pattern)
    assert (np.bincount(gpu @ np.array([1, 2, 4]), minlength=8) >= 16).all()
    for v in range(3):  # a view that does not see a Gaussian gives it no gradient, one that does gives one
        m = torch.from_numpy(gpu[:, v]).to(device)
        assert not c.per_view[v]["sh"][~m].any() and not c.per_view[v]["means3D"][~m].any()
        assert c.per_view[v]["sh"][m].flatten(1).any(1).float().mean() > 0.9
    for order in itertools.permutations(range(3)):
        for acc in (0, ALL, _C().GS_ACC["sh"], ALL & ~_C().GS_ACC["sh"]):
            pre = c.prefill("random")
            pay = c.prefill("payload")
            pre = {n: (pre[n] if acc & _C().GS_ACC[n] else pay[n]) for n in pre}
            got = c.fused({n: t.clone() for n, t in pre.items()}, acc, order=order)
            want = c.ref_a(pre, acc, order)
            for n in want:
                assert _same(got[n], want[n]), (D, order, acc, n, _first_diff(got[n], want[n]))


def test_visibility_scene_against_the_dense_reference(device):
    s = fvc.visibility_scene()
    c = _check_b(device, ("vis",), s.leaves, s.cams, 3)
    # the clamp cluster's red channel is clamped in view 2 and free in view 1: its dL/dsh (coefficient 0, red)
    # is view 0's and view 1's alone
    sel = torch.from_numpy(s.group == [g[0] for g in fvc.VIS_GROUPS].index("clamp")).to(device)
    assert not c.per_view[2]["sh"][sel][:, :, 0].any() and c.per_view[1]["sh"][sel][:, 0, 0].any()


# ------------------------------------------------------------------------------------------
# 5. input kinds
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M", [(1, 4), (3, 16), (2, 16)])
@pytest.mark.parametrize("acc", [0, ALL], ids=["written", "accumulated"])
def test_precomputed_covariance(device, D, M, acc):
    """cov3D_precomp: dL/dcov3D is the real output; scales / rotations buffers, if passed, are not touched."""
    c = _layout_case(device, 257, D, M, "cov3d")
    assert "cov3D" in c.names and "scales" not in c.names
    got = c.check_a(acc)
    assert got["cov3D"].any()
    extra = {"scales": _payload((c.P, 3), device), "rotations": _payload((c.P, 4), device)}
    pre = c.prefill("random" if acc else "payload")
    again = c.fused({**{n: t.clone() for n, t in pre.items()}, **extra}, acc)
    for n in c.names:
        assert _same(again[n], got[n]), n
    assert all((extra[n].view(torch.int32) == PAYLOAD).all() for n in extra)


@pytest.mark.parametrize("acc", [0, ALL], ids=["written", "accumulated"])
def test_scale_modifier(device, acc):
    c = _layout_case(device, 257, 2, 9, "sh", mod=0.7)
    c.check_a(acc)
    plain = _layout_case(device, 257, 2, 9, "sh")
    assert not _same(c.per_view[0]["scales"], plain.per_view[0]["scales"])  # the modifier is in the chain


def test_colours_accumulate_bit_alone(device):
    """Precomputed colours with GS_ACC["colors"] alone: that output adds to its prefill, the others are written."""
    c = _layout_case(device, 257, 0, 1, "colors")
    bit = _C().GS_ACC["colors"]
    pre = {n: (c.prefill("random")[n] if n == "colors" else c.prefill("payload")[n]) for n in c.names}
    got = c.fused({n: t.clone() for n, t in pre.items()}, bit)
    ref = c.ref_a(pre, bit)
    for n in ref:
        assert _same(got[n], ref[n]), (n, _first_diff(got[n], ref[n]))
    assert not _same(got["colors"], c.check_a(0)["colors"])


@pytest.mark.parametrize("missing", ["cov3D", "colors", "both"])
@pytest.mark.parametrize("D,M,kind", [(3, 16, "sh"), (2, 9, "sh"), (0, 1, "colors")], ids=["sh3_m16", "sh2_m9", "colors"])
def test_outs_without_cov3d_or_colours(device, host_path, D, M, kind, missing):
    """The optional outputs left out: the others are what they are with them."""
    c = _layout_case(device, 257, D, M, kind)
    gone = ("cov3D", "colors") if missing == "both" else (missing,)
    names = tuple(n for n in c.names if n not in gone)
    for acc in (0, ALL):
        full = c.check_a(acc)
        part = c.check_a(acc, names=names)
        assert set(part) == set(names)
        for n in names:
            assert _same(part[n], full[n]), (missing, acc, n)


# ------------------------------------------------------------------------------------------
# 6. SH input with no dL/dsh output
# ------------------------------------------------------------------------------------------
E_DSH = "dL_dsh is required with SHs"


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def test_sh_input_without_sh_output_is_refused(device, host_path):
    """SH colours chain into dL/dmeans3D through the view direction, in the kernels that form dL/dsh.  Without
    that output both backward entries used to run their colours kernel: a dL/dmeans3D without the term, with
    the clamp bits ignored.  Contract (include/gsrast.h): the combination is refused, nothing is written."""
    from diff_gaussian_rasterization import _native

    C, lib = _C(), _native.load()
    c = _layout_case(device, 257, 1, 4, "sh")
    L = c.L
    outs = {n: t for n, t in c.prefill("payload").items() if n != "sh"}
    with pytest.raises(RuntimeError, match=E_DSH):
        c.fused(outs, 0)
    torch.cuda.synchronize()
    assert all((t.view(torch.int32) == PAYLOAD).all() for t in outs.values())
    # the C entries
    arr = (_native.ViewGrad * len(c.views))()
    keep = []  # (the cameras' matrices are transposed views: the library reads contiguous ones)
    for k, (vm, pm, cp, tx, ty, W, H, geom) in enumerate(c.views):
        keep += [vm.contiguous(), pm.contiguous(), cp.contiguous()]
        arr[k] = _native.ViewGrad(*(t.data_ptr() for t in keep[-3:]), tx, ty, W, H, geom.data_ptr())
    o = c.prefill("payload")
    st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def grads(dsh):
        return (_p(o["colors"]), _p(o["opacity"]), _p(o["means3D"]), _p(o["cov3D"]), dsh, _p(o["scales"]),
                _p(o["rotations"]))

    scene = (_p(L["means3D"]), _p(L["shs"]), None, _p(L["scales"]), 1.0, _p(L["rotations"]), None)
    for acc in (0, ALL):
        assert lib.gs_backward_gaussians(c.P, c.D, c.M, *scene, len(c.views), arr, *grads(None), acc, None, 0, st) == 1
        assert _native.last_error() == E_DSH
        assert lib.gs_backward_gaussians_range(c.P, 3, 200, c.D, c.M, *scene, len(c.views), arr, *grads(None), acc, None,
                                               0, st) == 1
        assert _native.last_error() == E_DSH
    # the single-view entry, on a forward of its own
    cam = c.cams[0]
    s, (num, _, radii, geom, binb, imgb) = c._forward(cam)
    m2 = _payload((c.P, 3), device)
    scratch = torch.empty((lib.gs_grad_buffer_bytes(num),), dtype=torch.uint8, device=device)
    vm, pm = s.viewmatrix.contiguous(), s.projmatrix.contiguous()
    args = (c.P, c.D, c.M, _p(s.bg), cam.image_width, cam.image_height, _p(L["means3D"]), _p(L["shs"]), None,
            _p(L["opacities"]), _p(L["scales"]), 1.0, _p(L["rotations"]), None, _p(vm), _p(pm),
            _p(s.campos), s.tanfovx, s.tanfovy, _p(radii), _p(geom), num, _p(binb), _p(imgb), _p(c.dpix[0]), _p(scratch),
            _p(m2))
    assert lib.gs_backward_accumulate(*args, *grads(None), 0, None, 0, st) == 1 and _native.last_error() == E_DSH
    assert lib.gs_backward(*args, *grads(None), 0, st) == 1 and _native.last_error() == E_DSH
    torch.cuda.synchronize()
    assert all((t.view(torch.int32) == PAYLOAD).all() for t in (*o.values(), m2))
    # with the output, the same calls run: the whole-range entry equals reference A
    assert lib.gs_backward_gaussians(c.P, c.D, c.M, *scene, len(c.views), arr, *grads(_p(o["sh"])), 0, None, 0, st) == 0
    ref = c.ref_a(o, 0)
    for n in ref:
        assert _same(o[n], ref[n]), n


def test_deferred_bucket_with_frozen_sh(device):
    """GradBucket(defer=True) over every parameter but the SH rows (which take no gradient): the deferred
    pass still needs the SH chain for dL/dmeans3D (it used to run the colours kernel).  Bit for bit the
    per-view autograd gradients summed with += in view order."""
    import gs_view_parallel as vp
    from diff_gaussian_rasterization import GaussianRasterizer

    leaves = fvc.layout_scene(257, 2, 16)
    cams = fvc.ring_cameras(3)
    rasts = [GaussianRasterizer(gs_scenes.raster_settings_for(cam, 2, device=device)) for cam in cams]
    dpix = [gs_scenes.dl_dimage(cam.image_height, cam.image_width, seed=60 + v, scale=1.0).to(device)
            for v, cam in enumerate(cams)]
    shs = leaves["shs"].to(device)
    names = ("means3D", "opacities", "scales", "rotations")

    def params():
        return {n: leaves[n].to(device).clone().requires_grad_(True) for n in names}

    def render(r, p):
        m2 = torch.zeros_like(p["means3D"], requires_grad=True)
        return r(means3D=p["means3D"], means2D=m2, opacities=p["opacities"], shs=shs, scales=p["scales"],
                 rotations=p["rotations"])[0]

    ref = None
    for r, dp in zip(rasts, dpix):  # plain autograd, a fresh gradient per view
        p = params()
        render(r, p).backward(dp)
        if ref is None:
            ref = {n: p[n].grad.clone() for n in names}
        else:
            for n in names:
                ref[n] += p[n].grad
    p = params()
    b = vp.GradBucket([p[n] for n in names], lazy_zero=True, defer=True)
    b.zero_grad()
    for r, dp in zip(rasts, dpix):
        render(r, p).backward(dp)
    b.finalize()
    torch.cuda.synchronize()
    for n in names:
        assert _same(p[n].grad, ref[n]), (n, _first_diff(p[n].grad, ref[n]))
    b.close()
