"""(GPU) densify_and_prune on the constructed cases of tests/constructed_densify.py.

End to end: gs_train.densify_and_prune against the oracle on the device (same inputs, same
torch.cuda.manual_seed), with the bounds of tests/test_densify.py (everything bit-exact, the
children's xyz at rtol 1e-6 / atol 1e-6), and, independently of the oracle, against the builder:
row count P' and every copied row the builder's gather.  The largest xyz error relative to its
bound is printed per case (`xyz_err_over_bound`).

ABI level: gs_densify_classify / gs_densify_split_stds alone need 20 bytes per Gaussian, so the
block scan is compared with the builder's totals and block bases up to P = 5,000,000 (the scan's
sequential part, `per` = ceil(blocks / 1024) classify blocks per thread, only works for
P > 262,144: per 2 at 262,145, 3 at 524,289, 4 at 1M, 20 at 5M).  The flag byte is internal and
not looked at.
"""
import ctypes

import numpy as np
import pytest
import torch

import constructed_densify as CD
from oracle import densify_oracle as DO
from test_densify import LRS, _compare_models, _run_both

pytestmark = pytest.mark.gpu

STATE_GROUPS = {"all": CD.NAMES, "none": (), "some": ("xyz", "f_rest")}


def _drop_state_except(keep):
    def prepare(m):
        for grp in m.optimizer.param_groups:
            if grp["name"] not in keep:
                del m.optimizer.state[grp["params"][0]]
    return prepare


def _xyz_err_over_bound(ours, ref):
    a, b = ours._xyz.detach().double(), ref._xyz.detach().double()
    if a.numel() == 0:
        return 0.0
    return float(((a - b).abs() / (1e-6 + 1e-6 * b.abs())).max())


def _run_case(case, device, f_rest_k=15, state="all"):
    arrays = case.arrays(f_rest_k)
    groups = STATE_GROUPS[state]
    ours, ref = _run_both(arrays, device, *case.args(), seed=7, N=case.N, with_state=state != "none",
                          prepare=_drop_state_except(groups) if state == "some" else None)
    print(f"{case.name}: P {case.P} -> {case.P_out} totals {case.totals.tolist()} "
          f"xyz_err_over_bound {_xyz_err_over_bound(ours, ref):.4f}")
    assert ours._xyz.shape[0] == case.P_out
    _compare_models(ours, ref)
    CD.assert_outputs_from_builder(case, arrays, ours, groups)
    return arrays, ours, ref


SCENES = {
    **{f"lanes_{k}": (lambda k=k: CD.lanes_scene(k)) for k in ("keep", "clone", "split", "split_child_big")},
    "dead_wave": CD.dead_wave_scene,
    "split_wave": CD.split_wave_scene,
    "clone_block_split_block": CD.clone_block_split_block_scene,
    "first_block_only": lambda: CD.one_block_only_scene("first"),
    "last_block_only": lambda: CD.one_block_only_scene("last"),
    **{w: (lambda w=w: CD.empty_class_scene(w)) for w in CD.EMPTY_CLASS},
}


@pytest.mark.parametrize("name", list(SCENES))
def test_arrangements_and_empty_classes(device, name):
    _run_case(SCENES[name](), device)  # f_rest 45 floats wide: the all-split wave loops over 64 x 45


SIZES = (1, 63, 64, 65, 255, 256, 257, 65_537)
SCREENS = (20.0, None, -1.0)
STATES = ("all", "none", "some")
F_REST_K = (0, 3, 15)


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("P", SIZES)
def test_sizes(device, P, N):
    """Every P with every N; screen size, Adam state and f_rest width cycle so that each value
    meets each P at some N."""
    i = SIZES.index(P)
    _run_case(CD.sized_scene(P, N, SCREENS[(i + N) % 3]), device, F_REST_K[(i + 2 * N) % 3], STATES[(i // 3 + N) % 3])


@pytest.mark.parametrize("f_rest_k", F_REST_K)
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("N,screen", [(1, 20.0), (2, None), (3, 20.0), (2, -1.0), (2, 20.0)])
def test_every_kind_and_tie(device, N, screen, state, f_rest_k):
    _run_case(CD.edges_scene(N, screen), device, f_rest_k, state)


@pytest.mark.parametrize("P", [262_144, 262_145])
def test_scan_per_thread_ranges_end_to_end(device, P):
    """per 1 -> 2 with kinds that differ from block to block inside a scan thread's range; narrow
    f_rest so the case stays small."""
    case = CD.scan_scene(P, "blocks", N=2)
    assert case.per == (1 if P == 262_144 else 2)
    _run_case(case, device, f_rest_k=3)


@pytest.mark.parametrize("which", CD.EMPTY_RESULT)
@pytest.mark.parametrize("state", ["all", "none"])
def test_empty_result(device, which, state):
    """Everything pruned: the reference's empty model (zero-row parameters and moments of the right
    trailing shapes, zero-row statistics, groups re-keyed, step kept), and a FusedAdam step on it runs."""
    from gs_train import FusedAdam

    case = CD.empty_class_scene(which)
    assert case.P_out == 0
    arrays, ours, _ = _run_case(case, device, state=state)
    groups = []
    for grp, lr in zip(ours.optimizer.param_groups, LRS):
        n = grp["name"]
        p = grp["params"][0]
        assert p is getattr(ours, DO.ATTRS[DO.NAMES.index(n)])
        assert tuple(p.shape) == (0,) + arrays[n].shape[1:] and p.is_cuda
        st = ours.optimizer.state.get(p)
        assert (st is not None) == (state == "all")
        if st is not None:
            assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
            assert float(st["step"]) == 2.0
        groups.append({"params": [p], "lr": lr, "name": n})
    assert ours.xyz_gradient_accum.shape == (0, 1) and ours.denom.shape == (0, 1) and ours.max_radii2D.shape == (0,)
    opt = FusedAdam(groups, lr=0.0, eps=1e-15)
    for g in groups:
        p = g["params"][0]
        if state == "all":
            opt.state[p] = ours.optimizer.state[p]
        p.grad = torch.zeros_like(p)
    opt.step()
    torch.cuda.synchronize()
    for g in groups:
        assert float(opt.state[g["params"][0]]["step"]) == (3.0 if state == "all" else 1.0)


def test_no_split_leaves_the_generator_alone(device):
    from gs_train import densify_and_prune
    from test_densify import _model_from

    case = CD.empty_class_scene("no_split")
    assert case.totals[2] == 0
    for fn in (DO.densify_and_prune, densify_and_prune):
        m = _model_from(case.arrays(), device)
        torch.cuda.manual_seed(11)
        before = torch.cuda.get_rng_state(device)
        fn(m, *case.args(), case.N)
        assert torch.equal(before, torch.cuda.get_rng_state(device)), fn.__module__
        assert m._xyz.shape[0] == case.P_out


# ---------------------------------------------------------------- ABI level: classify + scan + stds

def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _classify_and_stds(case, device):
    from diff_gaussian_rasterization import _native

    lib = _native.load()
    P, N = case.P, case.N
    accum, denom, opacity, scaling = (torch.from_numpy(a).to(device) for a in case.decision_inputs())
    blocks = lib.gs_densify_block_count(P)
    assert blocks == case.blocks
    flags = torch.empty((P,), dtype=torch.uint8, device=device)
    counts = torch.full((4 * blocks,), -1, dtype=torch.int32, device=device)
    totals = torch.full((4,), -1, dtype=torch.int32, device=device)
    thr, min_op, extent, screen = case.args()
    st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    with torch.cuda.device(device):
        _native.check(lib.gs_densify_classify(
            P, _ptr(accum), _ptr(denom), _ptr(opacity), _ptr(scaling), float(thr), float(CD.PERCENT_DENSE * extent),
            float(min_op), float(0.1 * extent), 1 if screen else 0, float(screen) if screen else 0.0, N,
            _ptr(flags), _ptr(counts), _ptr(totals), st), "classify")
        tot = totals.cpu().numpy().astype(np.int64)
        np.testing.assert_array_equal(tot, case.totals)
        bases = counts.cpu().numpy().astype(np.int64).reshape(blocks, 4)
        bad = np.nonzero((bases != case.block_bases).any(1))[0]
        assert bad.size == 0, f"{bad.size} block bases differ, first at block {bad[0]}: " \
                              f"{bases[bad[0]]} != {case.block_bases[bad[0]]} (per {case.per})"
        n_split = int(tot[2])
        assert n_split > 0
        stds = torch.full((N * n_split, 3), float("nan"), dtype=torch.float32, device=device)
        tot_h = (ctypes.c_uint32 * 4)(*[int(v) for v in tot])
        _native.check(lib.gs_densify_split_stds(P, N, tot_h, _ptr(flags), _ptr(counts), _ptr(scaling), _ptr(stds),
                                                st), "stds")
        want = torch.exp(scaling)[torch.from_numpy(case.split).to(device)].repeat(N, 1)
        assert stds.shape == want.shape and torch.equal(stds, want)


@pytest.mark.parametrize("pattern", ["blocks", "random"])
@pytest.mark.parametrize("P", [262_144, 262_145, 524_288, 524_289, 1_000_000, 5_000_000])
def test_scan_bases_and_stds_at_large_P(device, P, pattern):
    case = CD.scan_scene(P, pattern, N=2 + (P % 2))
    assert case.per == {262_144: 1, 262_145: 2, 524_288: 2, 524_289: 3, 1_000_000: 4, 5_000_000: 20}[P]
    _classify_and_stds(case, device)
